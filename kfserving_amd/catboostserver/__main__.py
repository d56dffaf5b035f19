"""python -m kfserving_amd.catboostserver --model_dir D [--model_name M]
(shaped after the xgbserver entry point; the model directory holds model.json)."""
import argparse
import logging
import sys

from ..kfserving import kfserver
from . import CatBoostModel

DEFAULT_MODEL_NAME = "default"

parser = argparse.ArgumentParser(parents=[kfserver.parser])
parser.add_argument('--model_dir', required=True,
                    help='A URI pointer to the model directory')
parser.add_argument('--model_name', default=DEFAULT_MODEL_NAME,
                    help='The name that the model is served under.')
args, _ = parser.parse_known_args()

if __name__ == "__main__":
    model = CatBoostModel(args.model_name, args.model_dir)
    try:
        model.load()
    except Exception:
        ex_type, ex_value, _ = sys.exc_info()
        logging.error(f"fail to load model {args.model_name} from dir {args.model_dir}. "
                      f"exception type {ex_type}, exception msg: {ex_value}")
        model.ready = False
    kfserver.KFServer().start([model] if model.ready else [])
