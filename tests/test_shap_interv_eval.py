"""tests/shap_interv_eval.py, the brute-force reference of the interventional
contributions, pinned on a tree small enough to do by hand and by efficiency."""
import numpy as np

from tests import shap_cat_eval as sc
from tests import shap_interact_cases as ic
from tests import shap_interv_eval as iv


def test_hand_computed_stump():
    """x0 <= 0 ? (x1 <= 0 ? 1 : -2) : 4 with x = (-1, -1), z = (1, 1):
    v{} = f(z) = 4, v{0} = f(-1, 1) = -2, v{1} = f(1, -1) = 4, v{0,1} = f(x) = 1, so
    phi_0 = ((-2 - 4) + (1 - 4)) / 2 = -4.5 and phi_1 = ((4 - 4) + (1 + 2)) / 2 = 1.5.
    A second background row equal to x halves both and moves the bias to 2.5."""
    f = ic.hand_tree()
    x = np.array([[-1.0, -1.0]])
    got = iv.contributions(f, x, np.array([[1.0, 1.0]]))
    assert np.array_equal(got, [[-4.5, 1.5, 4.0]])
    got = iv.contributions(f, x, np.array([[1.0, 1.0], [-1.0, -1.0]]))
    assert np.array_equal(got, [[-2.25, 0.75, 2.5]])


def test_efficiency():
    f = sc.lgb_cat_forest(4, 9, 6, seed=31, cat_features=(1,), n_categories=40, K=3)
    X, Z = sc.rows(f, 5, seed=1, n_categories=40), sc.rows(f, 7, seed=2, n_categories=40)
    phi = iv.contributions(f, X, Z).reshape(5, 3, 7)
    fx = iv.margins(f, sc.decisions(f, X))
    np.testing.assert_allclose(phi.sum(axis=2), fx, rtol=0, atol=1e-12)
    assert not iv.contributions(f, X[:1], X[:1]).reshape(3, 7)[:, :6].any()   # x against itself
