"""LightGBM linear-tree models (``linear_tree=true``, LightGBM >= 3.2) on the
host: the loader's ``lin_*`` arrays, the writer, the generator, ``Forest``'s
checks and subsetting, and hand-computed answers for the CPU reference
(tests/linear_eval.py) the GPU tests compare against."""
import dataclasses

import numpy as np
import pytest

from kfserving_amd.forest import TI_F32
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats.lightgbm_format import LightGBMFormatError, parse_lightgbm_text

from tests import linear_eval

HEADER = """tree
version=v3
num_class=1
num_tree_per_iteration=1
label_index=0
max_feature_idx=3
objective=regression
feature_names=a b c d
feature_infos=none none none none
tree_sizes=0 0 0

"""

TREE0 = """Tree=0
num_leaves=2
num_cat=0
split_feature=0
split_gain=1
threshold=0.5
decision_type=2
left_child=-1
right_child=-2
leaf_value=0.25 -0.5
shrinkage=1


"""

# leaf 0 has no terms (the double blank), leaf 1 three
TREE1 = """Tree=1
num_leaves=2
num_cat=0
split_feature=1
split_gain=1
threshold=0
decision_type=2
left_child=-1
right_child=-2
leaf_value=1 2
is_linear=1
leaf_const=1.5 2.5
num_features=0 3
leaf_features= 2 0 3
leaf_coeff= 0.5 -2 4
shrinkage=1


"""

TREE2 = """Tree=2
num_leaves=1
num_cat=0
leaf_value=0.125
is_linear=1
leaf_const=0.375
num_features=0
leaf_features=
leaf_coeff=
shrinkage=1


"""

MODEL = HEADER + TREE0 + TREE1 + TREE2 + "end of trees\n"


def test_hand_written_model_arrays():
    f = parse_lightgbm_text(MODEL)
    assert f.has_linear and f.n_trees == 3 and f.n_features == 4
    # nodes: tree 0 = [split, leaf, leaf], tree 1 = [split, leaf, leaf], tree 2 = [leaf]
    assert f.tree_offset.tolist() == [0, 3, 6, 7]
    assert f.lin_offset.dtype == np.int64 and f.lin_offset.tolist() == [0, 0, 0, 0, 0, 0, 3, 3]
    assert f.lin_feature.dtype == np.int32 and f.lin_feature.tolist() == [2, 0, 3]
    assert f.lin_coeff.dtype == np.float64 and f.lin_coeff.tolist() == [0.5, -2.0, 4.0]
    # a constant tree: zero terms, lin_const = leaf_value
    assert f.lin_const.tolist() == [0.0, 0.25, -0.5, 0.0, 1.5, 2.5, 0.375]
    assert f.leaf_value[:, 0].tolist() == [0.0, 0.25, -0.5, 0.0, 1.0, 2.0, 0.125]
    f.validate()


def test_constant_model_has_no_linear_arrays():
    f = parse_lightgbm_text(HEADER + TREE0 + "end of trees\n")
    assert not f.has_linear
    assert f.lin_offset is None and f.lin_feature is None
    assert f.lin_coeff is None and f.lin_const is None
    g = parse_lightgbm_text(HEADER + TREE0.replace("shrinkage=1", "is_linear=0\nshrinkage=1")
                            + "end of trees\n")
    assert not g.has_linear


def test_n_features_covers_linear_terms():
    f = parse_lightgbm_text(MODEL.replace("leaf_features= 2 0 3", "leaf_features= 2 0 9"))
    assert f.n_features == 10


def _gen(n_trees=7, num_leaves=9, n_features=6, seed=3, **kw):
    trees = lf.synthetic_leafwise_trees(n_trees, num_leaves, n_features, seed=seed)
    return lf.add_linear_leaves(trees, n_features, seed + 1, **kw)


def test_generator_is_seeded_and_mixed():
    a = _gen(max_terms=3, const_tree_every=3)
    b = _gen(max_terms=3, const_tree_every=3)
    assert ["leaf_const" in t for t in a] == [False, True, True, False, True, True, False]
    counts = []
    for ta, tb in zip(a, b):
        if "leaf_const" not in ta:
            continue
        assert np.array_equal(ta["leaf_const"], tb["leaf_const"])
        for fa, fb, ca, cb in zip(ta["leaf_features"], tb["leaf_features"],
                                  ta["leaf_coeff"], tb["leaf_coeff"]):
            assert np.array_equal(fa, fb) and np.array_equal(ca, cb)
            assert len(set(fa.tolist())) == len(fa) <= 3 and len(fa) == len(ca)
            assert fa.size == 0 or (fa.min() >= 0 and fa.max() < 6)
            counts.append(len(fa))
    assert 0 in counts and 3 in counts


def test_writer_loader_round_trip(tmp_path):
    trees = _gen(max_terms=4, const_tree_every=3)
    path = str(tmp_path / "m.txt")
    lf.write_lightgbm_text(path, trees, 6, "regression")
    f = lf.load_lightgbm_model(path)
    f.validate()
    assert f.has_linear
    for t, tr in enumerate(trees):
        s = f.tree_slice(t)
        nl = len(tr["leaf_value"])
        leaves = range(s.stop - nl, s.stop)          # leaf j is node n_int + j
        assert np.all(np.diff(f.lin_offset[s.start:s.stop - nl + 1]) == 0)
        for j, n in enumerate(leaves):
            a, b = int(f.lin_offset[n]), int(f.lin_offset[n + 1])
            assert f.leaf_value[n, 0] == tr["leaf_value"][j]
            if "leaf_const" not in tr:
                assert a == b and f.lin_const[n] == tr["leaf_value"][j]
                continue
            assert f.lin_const[n] == tr["leaf_const"][j]
            assert f.lin_feature[a:b].tolist() == tr["leaf_features"][j].tolist()
            assert f.lin_coeff[a:b].tolist() == tr["leaf_coeff"][j].tolist()


def test_writer_blanks_of_empty_leaves(tmp_path):
    tree = {"split_feature": [0], "threshold": [0.5], "decision_type": [2], "left_child": [-1],
            "right_child": [-2], "leaf_value": [1.0, 2.0], "leaf_const": [1.5, 2.5],
            "leaf_features": [np.array([], np.int64), np.array([2, 0])],
            "leaf_coeff": [np.array([]), np.array([0.5, -2.0])]}
    path = str(tmp_path / "m.txt")
    lf.write_lightgbm_text(path, [tree], 3, "regression")
    lines = open(path).read().split("\n")
    at = lines.index("is_linear=1")
    assert lines[at - 1] == "leaf_value=1.0 2.0"
    assert lines[at + 1:at + 6] == ["leaf_const=1.5 2.5", "num_features=0 2",
                                    "leaf_features= 2 0  ", "leaf_coeff= 0.5 -2.0  ",
                                    "shrinkage=1"]


def test_writer_unchanged_without_linear_keys(tmp_path):
    tree = {"split_feature": [1], "threshold": [0.25], "decision_type": [10], "left_child": [-1],
            "right_child": [-2], "leaf_value": [0.5, -1.0], "leaf_count": [3, 4],
            "internal_count": [7]}
    path = str(tmp_path / "m.txt")
    lf.write_lightgbm_text(path, [tree, {"leaf_value": [0.125]}], 2, "binary sigmoid:1")
    want = "\n".join([
        "tree", "version=v3", "num_class=1", "num_tree_per_iteration=1", "label_index=0",
        "max_feature_idx=1", "objective=binary sigmoid:1", "feature_names=Column_0 Column_1",
        "feature_infos=none none", "tree_sizes=0 0", "",
        "Tree=0", "num_leaves=2", "num_cat=0", "split_feature=1", "split_gain=1",
        "threshold=0.25", "decision_type=10", "left_child=-1", "right_child=-2",
        "leaf_value=0.5 -1.0", "leaf_count=3 4", "internal_count=7", "shrinkage=1", "", "",
        "Tree=1", "num_leaves=1", "num_cat=0", "leaf_value=0.125", "shrinkage=1", "", "",
        "end of trees", ""])
    assert open(path).read() == want


@pytest.mark.parametrize("old,new", [
    ("leaf_features= 2 0 3", "leaf_features= 2 0"),                 # short token list
    ("leaf_coeff= 0.5 -2 4", "leaf_coeff= 0.5 -2"),                 # short token list
    ("leaf_features= 2 0 3", "leaf_features= 2 0 3 1"),             # long token list
    ("leaf_coeff= 0.5 -2 4", "leaf_coeff= 0.5 -2 4 8"),             # long token list
    ("leaf_const=1.5 2.5", "leaf_const=1.5 2.5 3.5"),               # wrong length
    ("leaf_const=1.5 2.5", "leaf_const=1.5"),                       # wrong length
    ("num_features=0 3", "num_features=0 3 0"),                     # wrong length
    ("num_features=0 3", "num_features=-1 4"),                      # negative m_j
    ("leaf_features= 2 0 3", "leaf_features= 2 -1 3"),              # negative feature
], ids=["short-features", "short-coeff", "long-features", "long-coeff", "const-long",
        "const-short", "counts-long", "negative-count", "negative-feature"])
def test_malformed_linear_block(old, new):
    assert old in MODEL
    with pytest.raises(LightGBMFormatError):
        parse_lightgbm_text(MODEL.replace(old, new))


def test_forest_validate_rejections():
    base = parse_lightgbm_text(MODEL)
    base.validate()

    def bad(**kw):
        with pytest.raises(ValueError):
            dataclasses.replace(base, **kw).validate()

    bad(lin_offset=base.lin_offset[:-1])                                  # length
    bad(lin_const=base.lin_const[:-1])                                    # length
    bad(lin_coeff=base.lin_coeff[:-1])                                    # length
    bad(lin_offset=np.array([0, 0, 0, 0, 0, 0, 3, 2], dtype=np.int64))    # does not end at M
    bad(lin_offset=np.array([0, 0, 0, 0, 0, 4, 3, 3], dtype=np.int64))    # not monotone
    bad(lin_offset=np.array([0, 0, 0, 0, 1, 1, 3, 3], dtype=np.int64))    # terms on a split
    bad(lin_feature=np.array([2, 0, 4], dtype=np.int32))                  # >= n_features
    bad(lin_feature=np.array([2, -1, 3], dtype=np.int32))                 # < 0
    bad(lin_const=None)                                                   # partial set
    bad(accum_dtype=TI_F32)                                               # float32 sums
    bad(n_groups=2, leaf_width=2, base_margin=np.zeros(2),
        leaf_value=np.zeros((base.n_nodes, 2)))                           # vector leaves


def _canonical_tree_outputs(f, X):
    """Per-tree outputs of a canonical linear forest, restated at the
    canonical level: a scalar walk of the node arrays (numerical splits with
    the NaN / zero flags), then the leaf's CSR range."""
    X = np.asarray(X, dtype=np.float64)
    Xz = np.where((np.abs(X) > float(np.float32(1e-35))) | np.isnan(X), X, 0.0)
    out = np.zeros((X.shape[0], f.n_trees))
    for r in range(X.shape[0]):
        for t in range(f.n_trees):
            b = int(f.tree_offset[t])
            n = b
            while f.feature[n] >= 0:
                x, thr, fl = Xz[r, f.feature[n]], f.threshold[n], int(f.flags[n])
                if np.isnan(x):
                    left = bool(fl & 1)
                elif x == 0 and (fl & 2):
                    left = not (0 <= thr)
                else:
                    left = x <= thr
                n = b + int(f.left[n] if left else f.right[n])
            acc, nan_found = f.lin_const[n], False
            for i in range(int(f.lin_offset[n]), int(f.lin_offset[n + 1])):
                v = Xz[r, f.lin_feature[i]]
                nan_found |= bool(np.isnan(v))
                acc = acc + f.lin_coeff[i] * v
            out[r, t] = f.leaf_value[n, 0] if nan_found else acc
    return out


def test_tree_subset_keeps_per_tree_outputs(tmp_path):
    trees = _gen(n_trees=9, max_terms=3, const_tree_every=4)
    path = str(tmp_path / "m.txt")
    lf.write_lightgbm_text(path, trees, 6, "regression")
    f = lf.load_lightgbm_model(path)
    rng = np.random.default_rng(8)
    X = rng.standard_normal((40, 6))
    X[rng.random(X.shape) < 0.1] = np.nan
    want, fell, _ = linear_eval.tree_outputs(open(path).read(), X)
    assert fell.any() and not fell.all()
    whole = _canonical_tree_outputs(f, X)
    assert linear_eval.same_bits(whole, want)
    for t0, t1 in ((0, 4), (4, 9), (3, 5), (8, 9)):
        sub = f.tree_subset(t0, t1).contiguous()
        sub.validate()
        assert sub.n_trees == t1 - t0 and sub.has_linear
        assert sub.lin_offset[0] == 0 and sub.lin_offset[-1] == sub.lin_feature.shape[0]
        assert linear_eval.same_bits(_canonical_tree_outputs(sub, X), want[:, t0:t1])


def test_linear_eval_hand_computed():
    """Tree 1 of MODEL: b <= 0 -> leaf 0 (1.5, no terms); else leaf 1:
    2.5 + 0.5 c - 2 a + 4 d, falling back to 2 on a NaN in c, a or d."""
    text = HEADER + TREE1.replace("Tree=1", "Tree=0") + "end of trees\n"
    inf, nan = np.inf, np.nan
    X = np.array([
        # a     b     c     d
        [1.0, 1.0, 3.0, 0.25],      # plain: 2.5 + 1.5 - 2 + 1 = 3
        [1.0, 1.0, nan, 0.25],      # NaN at the first term: fallback 2
        [1.0, 1.0, 3.0, nan],       # NaN at the last term: fallback 2
        [1.0, nan, 3.0, 0.25],      # NaN only in b, which no term reads; the split
                                    # (missing type None: NaN reads 0) goes to leaf 0
        [1.0, -1.0, nan, nan],      # leaf 0 has no terms: NaNs are not read at all
        [0.0, 1.0, 0.0, 1e-36],     # zero map: the d term is 0, not 4e-36
    ])
    out, fell, leaves = linear_eval.tree_outputs(text, X)
    assert leaves[:, 0].tolist() == [1, 1, 1, 0, 0, 1]
    assert out[:, 0].tolist() == [3.0, 2.0, 2.0, 1.5, 1.5, 2.5]
    assert fell[:, 0].tolist() == [False, True, True, False, False, False]


SIX_ROWS_TEXT = (HEADER.replace("tree_sizes=0 0 0", "tree_sizes=0") + """Tree=0
num_leaves=2
num_cat=0
split_feature=0
split_gain=1
threshold=0
decision_type=2
left_child=-1
right_child=-2
leaf_value=-7 7
is_linear=1
leaf_const=0.5 0.25
num_features=2 2
leaf_features=1 2  1 2
leaf_coeff=1e+38 0.0  2.0 -4.0
shrinkage=1


end of trees
""")

# the six rows of the issue, float32-representable: feature 3 is read by nothing
SIX_ROWS = np.array([
    # a     b        c       d
    [1.0, 3.0, 0.5, 1.0],            # plain: 0.25 + 6 - 2 = 4.25
    [1.0, np.nan, 0.5, 1.0],         # NaN at the first term: fallback 7
    [1.0, 3.0, np.nan, 1.0],         # NaN at the last term: fallback 7
    [1.0, 3.0, 0.5, np.nan],         # NaN only in the unused feature: 4.25, no fallback
    [-1.0, 1e-36, 2.0, 1.0],         # leaf 0: 1e38 * zero-mapped 1e-36 = 0, not 100 -> 0.5
    [-1.0, 2.0, np.inf, 1.0],        # leaf 0: 0.5 + 2e38 + 0.0 * inf = NaN score
])
SIX_WANT = np.array([4.25, 7.0, 7.0, 4.25, 0.5, np.nan])
SIX_FELL = [False, True, True, False, False, False]


def test_linear_eval_six_rows():
    for dt in (np.float64, np.float32):
        X = SIX_ROWS.astype(dt)
        score, fell = linear_eval.raw_scores(SIX_ROWS_TEXT, X)
        assert linear_eval.same_bits(score[:, 0], SIX_WANT)
        assert np.isnan(score[5, 0])
        assert fell[:, 0].tolist() == SIX_FELL
