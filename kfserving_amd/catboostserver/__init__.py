from .model import CatBoostModel  # noqa: F401
