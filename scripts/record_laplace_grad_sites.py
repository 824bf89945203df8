#!/usr/bin/env python
"""Records tests/golden/laplace_grad_sites_parent.npz (tests/laplace_grad_sites.py describes it) on the GPU.

Run it ONLY against a library built from the commit whose results are the reference -- the parent of a change that must not move a bit:

    python scripts/record_laplace_grad_sites.py <commit hash of the library's source> [output.npz]

The values are collected twice, each time in a process of its own: `a/<name>` and `b/<name>`.  Where the two agree bit for bit the test asks for those bits;
where they differ it asks for the parent's own spread.  The refusals' messages are stored once (`refusal/<name>`); the two recordings must agree on them.  The
library is the one gpboost_amd loads (GPBOOST_AMD_LIB overrides the path)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import laplace_grad_sites as S   # noqa: E402


def record_once(path):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "the recorder needs the MI355X"
    gpboost_amd.set_device(0)
    vals = S.collect()
    assert sorted(vals) == sorted(S.NAMES), sorted(set(vals) ^ set(S.NAMES))
    msgs = S.refusals()
    assert sorted(msgs) == sorted(S.REFUSALS) and all(msgs.values()), msgs
    vals.update({"refusal/" + k: np.array(v) for k, v in msgs.items()})
    np.savez(path, **vals)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--once":
        return record_once(sys.argv[2])
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    commit = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", S.FIXTURE)
    data = {"parent": np.array(commit)}
    with tempfile.TemporaryDirectory() as tmp:
        for tag in ("a", "b"):
            one = os.path.join(tmp, tag + ".npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--once", one], timeout=300)
            with np.load(one) as f:
                for k in f.files:
                    if not k.startswith("refusal/"):
                        data[tag + "/" + k] = f[k]
                    elif tag == "a":
                        data[k] = f[k]
                    else:
                        assert str(data[k]) == str(f[k]), (k, str(data[k]), str(f[k]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **data)
    same = [k for k in S.NAMES if np.array_equal(data["a/" + k].view(np.uint64), data["b/" + k].view(np.uint64))]
    print("wrote %s: %d quantities, %d refusals, %d bytes, commit %s" % (out_path, len(S.NAMES), len(S.REFUSALS), os.path.getsize(out_path), commit))
    print("bit for bit in both recordings: %d of %d" % (len(same), len(S.NAMES)))
    for k in S.NAMES:
        if k not in same:
            a, b = data["a/" + k], data["b/" + k]
            print("differs between the recordings: %s by %.3e (relative to its largest magnitude)" % (k, np.abs(a - b).max() / np.abs(a).max()))
    for k in S.REFUSALS:
        print("refusal %s: %s" % (k, str(data["refusal/" + k])))


if __name__ == "__main__":
    main()
