#!/usr/bin/env python3
"""Per-kernel resources of device assembly: one JSON line per kernel symbol.

    hipcc <HIP_FLAGS of __graft_entry__.py> -I include -I kfserving_amd/csrc \\
          --cuda-device-only -S kfserving_amd/csrc/treeinfer_k_fd.hip -o k_fd.s
    scripts/kernel_resources.py k_*.s > table.jsonl
    scripts/kernel_resources.py --compare parent.jsonl table.jsonl

Each line is a JSON array in the order of COLUMNS: the symbol, the registers,
scratch, occupancy and code length the compiler reports for it, and a hash of
its instruction lines (comments dropped, local label numbers stripped; the
first 16 hex digits of their SHA-256), so two builds of the same kernels can
be compared without a GPU: equal hashes are the same code.  --compare exits 1
when the symbol sets differ or a kernel's VGPRs, SGPRs, scratch or occupancy
do.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")
SYMBOL = re.compile(r"^([A-Za-z_][\w$.]*):")
DIRECTIVES = {".amdhsa_next_free_vgpr": "vgpr", ".amdhsa_next_free_sgpr": "sgpr",
              ".amdhsa_private_segment_fixed_size": "private_segment"}
INFO = {"codeLenInByte": "code_bytes", "ScratchSize": "scratch", "Occupancy": "occupancy"}
GATED = ("vgpr", "sgpr", "private_segment", "scratch", "occupancy")
COLUMNS = ("kernel",) + GATED + ("code_bytes", "hash")   # a table line, as an array


def kernels(path):
    """Yield one record per .amdhsa_kernel of the assembly file."""
    body = {}          # symbol -> sha256 of its instruction lines
    sym, sha, rec = None, None, None
    with open(path, errors="replace") as fh:
        for raw in fh:
            line = raw.split(";", 1)[0].strip()
            if rec is not None and raw.startswith(";"):
                m = re.match(r";\s*(\w+)\s*[:=]\s*(\d+)", raw)
                if m and m.group(1) in INFO:
                    rec[INFO[m.group(1)]] = int(m.group(2))
                    if m.group(1) == "Occupancy":   # the last figure of a kernel's block
                        yield rec
                        rec = None
                continue
            if not line:
                continue
            m = SYMBOL.match(raw)
            if m and not raw.startswith(".L"):
                sym, sha = m.group(1), hashlib.sha256()
                continue
            word = line.split(None, 1)
            if word[0] == ".section" and sym is not None:   # the function's text is over
                body[sym] = sha.hexdigest()[:16]
                sym = None
            elif word[0] == ".amdhsa_kernel":
                rec = {"kernel": word[1], "hash": body.get(word[1])}
            elif rec is not None and word[0] in DIRECTIVES:
                rec[DIRECTIVES[word[0]]] = int(word[1])
            elif sym is not None and (not line.startswith(".") or line.startswith(".L")):
                sha.update(LABEL.sub(".L", line).encode() + b"\n")   # directives are skipped


def load(path):
    with open(path) as fh:
        return {r[0]: dict(zip(COLUMNS, r)) for r in map(json.loads, fh) if r}


def compare(parent_path, new_path):
    parent, new = load(parent_path), load(new_path)
    bad = 0
    for k in sorted(set(parent) ^ set(new)):
        print(("only in parent: " if k in parent else "only in new: ") + k)
        bad += 1
    same_hash = 0
    for k in sorted(set(parent) & set(new)):
        p, n = parent[k], new[k]
        diff = [f"{g} {p.get(g)} -> {n.get(g)}" for g in GATED if p.get(g) != n.get(g)]
        if diff:
            print(f"{k}: " + ", ".join(diff))
            bad += 1
        same_hash += p["hash"] == n["hash"]
    both = len(set(parent) & set(new))
    print(f"{both} kernels in both, {same_hash} with the same instruction hash, "
          f"{both - same_hash} changed, {bad} outside the conditions")
    for k in sorted(set(parent) & set(new)):
        if parent[k]["hash"] != new[k]["hash"]:
            print(f"changed: {k} code_bytes {parent[k].get('code_bytes')} -> {new[k].get('code_bytes')}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--compare", action="store_true", help="compare two tables instead")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    if args.compare:
        if len(args.files) != 2:
            ap.error("--compare takes the parent's table and the new one")
        return compare(*args.files)
    for path in args.files:
        for rec in kernels(path):
            print(json.dumps([rec.get(c) for c in COLUMNS], separators=(",", ":")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
