#!/usr/bin/env python
"""Records tests/golden/point_kernel_bits.npz (tests/point_kernel_bits.py describes it) on the GPU.

Run it ONLY against a library built from the commit whose results are the reference -- the parent of a change that must not move a bit:

    python scripts/record_point_kernel_bits.py <commit hash of the library's source> [output.npz]

The library is the one gpboost_amd loads (GPBOOST_AMD_LIB overrides the path)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import point_kernel_bits as B   # noqa: E402


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    commit = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", B.FIXTURE)
    import gpboost_amd
    from gpboost_amd.libpath import find_lib_path
    assert gpboost_amd.device_count() > 0, "the recorder needs the MI355X"
    gpboost_amd.set_device(0)
    data = {"parent": commit, "exp2_table": B.host_exp2_table()}
    for case in B.cases():
        data.update(B.collect(case))
        print("recorded", case.id, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    B.save(out_path, data)
    print("wrote %s: %d values, %d bytes, library %s, commit %s" % (out_path, len(data), os.path.getsize(out_path), find_lib_path(), commit))


if __name__ == "__main__":
    main()
