"""Build an A/B variant of libtreeinfer.so into kfserving_amd/lib/variants/NAME/
(git-ignored; it travels to the GPU box with the tree), for
scripts/ab_libraries.py and scripts/runs/ab_variant.sh:

    python scripts/build_variant.py NAME [--source DIR] [-D...]

The extra flags (-DTI_TILP=4 ...) go to every unit.  --source DIR compiles the
sources of another checkout of this repository (its kfserving_amd/csrc and
include), for instance a `git worktree add DIR <commit>` of the parent commit:
that is how a side with an earlier kernel is made.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    import __graft_entry__ as g
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("name")
    ap.add_argument("--source", help="root of the checkout to compile (default: this one)")
    args, flags = ap.parse_known_args()
    if args.source:
        g.ROOT = os.path.abspath(args.source)
        g.CSRC = os.path.join(g.ROOT, "kfserving_amd", "csrc")
    out = os.path.join(ROOT, "kfserving_amd", "lib", "variants", args.name, "libtreeinfer.so")
    print(g.build_library(verbose=True, extra_flags=flags, lib=out))
