"""C2 fixed walk: LDS cycles per 32-lane group of a ds_read_b64 pair read
(64 banks, MI355X_MICROARCH.md LDS) with heap-ordered, cover-permuted
(sequential slots, hottest first) and bank-spread pair slots (fix_permute's
default: levels of more than 32 pairs give each node, hottest first, the
least-loaded of the 32 bank classes that still has room).
Usage: python scripts/sim/c2_pair_banks.py [n_trees]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from kfserving_amd.formats import xgboost_format as xf
trees, ti = xf.synthetic_complete_trees(int(sys.argv[1]) if len(sys.argv) > 1 else 100, 8, 28, seed=0)
rng = np.random.default_rng(1000)
R = 4096
X = rng.standard_normal((R, 28)).astype(np.float32)
NAMES = ("plain", "permuted", "spread")
tot = np.zeros((3, 8)); n = np.zeros(8)
for t in trees:
    cl, cr, si, val, hs = t['cleft'], t['cright'], t['sindex'], t['value'], t['sum_hess']
    feat = si & 0x7FFFFFFF
    # heap index h (1-based) <-> node id v = h - 1
    # permutation per level by hess desc: sequential slots, and spread over
    # the 32 bank classes (slot s is in class s % 32)
    pi = np.zeros((3, 256), np.int64)
    pi[0] = np.arange(256)
    for lo in [1 << l for l in range(8)]:
        hs_l = hs[np.arange(lo, 2 * lo) - 1]
        order = np.argsort(-hs_l, kind='stable')
        pi[1, lo + order] = lo + np.arange(lo)
        if lo <= 32:
            pi[2, lo + order] = lo + np.arange(lo)
            continue
        load = np.zeros(32); used = np.zeros(32, np.int64)
        for i in order:
            free = np.nonzero(used < lo // 32)[0]
            k = free[np.argmin(load[free])]          # ties: the lowest class
            pi[2, lo + i] = lo + k + 32 * used[k]
            load[k] += hs_l[i]; used[k] += 1
    h = np.ones(R, np.int64)
    for l in range(8):
        v = h - 1
        x = X[np.arange(R), feat[v]]
        right = ~(x < val[v])
        # pair read of node h at level l (levels 1..7 read from LDS; level 0 is scalar)
        if l >= 1:
            for perm in range(3):
                dw = 2 * pi[perm, h]            # dword index of the pair
                for g in range(R // 32):
                    d = np.unique(dw[g*32:(g+1)*32])
                    banks = np.concatenate([d % 64, (d + 1) % 64])
                    tot[perm, l] += np.bincount(banks, minlength=64).max()
            n[l] += R // 32
        h = 2 * h + right
for perm in range(3):
    print("avg LDS cycles per 32-lane group of a pair read, %-8s: %.3f (1.0 = conflict-free); levels 1-7: %s"
          % (NAMES[perm], tot[perm].sum() / n.sum(),
             " ".join("%.2f" % (tot[perm, l] / n[l]) for l in range(1, 8))))
