"""What tests/golden/point_kernel_bits.npz holds and how it is produced: the bit patterns of everything vecchia_point_kernel (gpboost_amd/csrc/vecchia_kernels.hip)
hands back, for every case of vecchia_point_ref.instance_cases() and latent_cases().  scripts/record_point_kernel_bits.py writes the file from a library built
at the commit whose results are the reference; tests/test_zz_point_kernel_bits_gpu.py runs the same function on the library under test and compares.

The file holds four arrays -- names, kinds (0: uint8, 1: uint64), lengths (bytes) and one blob with every value back to back (a zip member per value
would cost more than the values) -- and `parent`; load() turns them back into {name: array}.  The names (case id = Case.id, shard "i0-i1", cap =
gpb_hip_vecchia_set_worker_cap):
    parent                      the commit the library was built from
    exp2_table                  uint64[256]: exp2(j / 256) of the libm the library links (the kernel's table is filled from it on the host)
    <id>/D, <id>/u              uint64[n]: the factor's D and u of the whole range with the default grid
    <id>/<shard>/c<cap>/A       uint8[32]: SHA-256 of the bytes of A[i0:i1]
    <id>/<shard>/c<cap>/Du      uint8[32]: SHA-256 of the bytes of D[i0:i1] followed by u[i0:i1]
    <id>/<shard>/c<cap>/nll     uint64[3]: nll_terms
    <id>/<shard>/c<cap>/grad    uint64[7]: grad_terms (Gaussian cases only)
"""
import ctypes
import hashlib

import numpy as np

from tests import vecchia_point_ref as R

FIXTURE = "point_kernel_bits.npz"
CAPS = (0, 2)


def save(path, data):
    names = sorted(k for k in data if k != "parent")
    arrs = [np.ascontiguousarray(data[k]) for k in names]
    assert all(a.dtype in (np.uint8, np.uint64) for a in arrs)
    np.savez_compressed(path, parent=np.array(str(data["parent"])), names=np.array(names), kinds=np.array([a.dtype == np.uint64 for a in arrs], dtype=np.uint8),
                        lengths=np.array([a.nbytes for a in arrs], dtype=np.int64), blob=np.frombuffer(b"".join(a.tobytes() for a in arrs), dtype=np.uint8))


def load(path):
    with np.load(path) as f:
        out = {"parent": str(f["parent"])}
        blob, at = f["blob"].tobytes(), 0
        for name, kind, nbytes in zip(f["names"], f["kinds"], f["lengths"]):
            out[str(name)] = np.frombuffer(blob[at:at + int(nbytes)], dtype=np.uint64 if kind else np.uint8)
            at += int(nbytes)
    return out


def cases():
    return R.instance_cases() + R.latent_cases()


def shards(case):
    return ((0, case.n), (7, case.n - 9))


def host_exp2_table():
    """exp2(j / 256), j = 0..255, from the libm that lib_gpboost_amd.so links (dlsym on the library's handle searches its dependencies)"""
    from gpboost_amd.libpath import find_lib_path
    lib = ctypes.CDLL(find_lib_path())
    f = lib.exp2
    f.restype = ctypes.c_double
    f.argtypes = [ctypes.c_double]
    return np.array([f(j / 256.0) for j in range(256)], dtype=np.float64).view(np.uint64)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def collect(case):
    """-> {key: array} of one case, from the library that gpboost_amd loads"""
    from gpboost_amd import shim
    cd = R.case_data(case)
    st = shim.VecchiaState(cd.coords, case.m)
    st.set_neighbors(cd.nn)
    st.set_y(cd.y)
    if case.wt:
        st.set_nugget_diag(cd.nug)
    out = {}
    for i0, i1 in shards(case):
        st.set_shard(i0, i1)
        for cap in CAPS:
            st.set_worker_cap(cap)
            key = "%s/%d-%d/c%d/" % (case.id, i0, i1, cap)
            st.factor(case.cov, case.var, case.a, gauss=case.gauss)
            A, D, u = st.get_factor()
            out[key + "A"] = _sha(A[i0:i1])
            out[key + "Du"] = _sha(D[i0:i1], u[i0:i1])
            if (i0, i1, cap) == (0, case.n, 0):
                out[case.id + "/D"] = D.view(np.uint64).copy()
                out[case.id + "/u"] = u.view(np.uint64).copy()
            out[key + "nll"] = st.nll_terms(case.cov, case.var, case.a, gauss=case.gauss).view(np.uint64).copy()
            if case.gauss:
                out[key + "grad"] = st.grad_terms(case.cov, case.var, case.a).view(np.uint64).copy()
    st.set_worker_cap(0)
    st.close()
    return out
