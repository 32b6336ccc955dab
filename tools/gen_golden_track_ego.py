"""Writes tests/golden/track_ego_unposed.npz: what tracking.Tracker gives, WITHOUT poses, on the sequences of
tests/track_ego_cases.unposed_cases -- per case the sha256 of every step's tracks() bytes and the last step's arrays.

The committed file was written from the tracker as it stood before it took poses (the commit before the ego-motion carry):
tests/test_track_ego_host.py holds the unposed path of every later tracker to those bytes.  Run from the repository root
of the checkout whose tracker is to be recorded; --root names another checkout to take pp_amd from.

    python tools/gen_golden_track_ego.py [--root DIR] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "track_ego_unposed.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(a.root))
    import pp_amd
    import track_ego_cases as C
    from pp_amd.engine import DET_DTYPE
    out = {}
    for name in C.unposed_cases():
        digest, (tr, n, ov) = C.run_unposed(pp_amd.tracking, DET_DTYPE, name)
        out[name + "/sha256"] = np.frombuffer(bytes.fromhex(digest), np.uint8)
        m = max(int(n.max()), 1)
        out[name + "/tracks"] = tr[:, :m]
        out[name + "/n"] = n
        out[name + "/overflow"] = ov
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {len(C.unposed_cases())} cases, {os.path.getsize(a.out)} bytes, tracker of {os.path.dirname(pp_amd.__file__)}")


if __name__ == "__main__":
    main()
