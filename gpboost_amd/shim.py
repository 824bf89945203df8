"""ctypes view of the low-level C ABI (include/gpb_hip.h): what the reference's C++ host would call.

``VecchiaState`` and ``HistBuilder`` are thin RAII wrappers; every method is one C call.  Used by the
parity tests and by bench.py (resident and sharded evaluation); the high-level mirror of the
reference's Python API is :class:`gpboost_amd.GPModel`.
"""
import ctypes as C

import numpy as np

from .basic import GPBoostError, _lib, _shim_call

MODE_NLL, MODE_FACTOR, MODE_GRAD = 0, 1, 2

# likelihoods of the Vecchia-Laplace path, name -> (id of gpb_hip_vecchia_laplace_set_likelihood, number of auxiliary parameters): the rows of
# csrc/lik_table.h (a test holds the two together).  The proportion likelihoods are the Bernoulli kernels with a real-valued response.
_LIKELIHOODS = {"bernoulli_logit": (0, 0), "bernoulli_probit": (1, 0), "poisson": (2, 0), "gamma": (3, 1), "negative_binomial": (4, 1), "beta": (5, 1),
                "t": (6, 2), "lognormal": (7, 1), "gaussian_latent": (8, 1)}
_LIKELIHOODS.update({prefix + link: _LIKELIHOODS["bernoulli_" + link] for prefix in ("binomial_", "quasi_bernoulli_") for link in ("logit", "probit")})


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


class VecchiaState(object):
    """coords: (n, d) array ALREADY in Vecchia order; m: number of neighbours."""

    def __init__(self, coords, m):
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim == 1:
            coords = coords.reshape(-1, 1)
        self.n, self.d = coords.shape
        self.m = max(min(int(m), self.n - 1), 1)
        cm = np.asfortranarray(coords)
        self.h = C.c_void_p()
        _shim_call(_lib().gpb_hip_vecchia_create(C.c_int(self.n), C.c_int(self.d), C.c_int(int(m)), _p(cm),
                                                 C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value is not None:
            _lib().gpb_hip_vecchia_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_handle(cls, ptr, n, d, m):
        """Non-owning view of a gpb_hip_vecchia_t* owned by a GPModel (GPB_HIP_GetVecchiaHandle)."""
        self = cls.__new__(cls)
        self.n, self.d, self.m = int(n), int(d), int(m)
        self.h = C.c_void_p(ptr.value if isinstance(ptr, C.c_void_p) else int(ptr))
        self.close = lambda: None
        return self

    def set_stream(self, hip_stream_ptr):
        _shim_call(_lib().gpb_hip_vecchia_set_stream(self.h, C.c_void_p(int(hip_stream_ptr))))

    def find_neighbors(self):
        dup = C.c_int(0)
        _shim_call(_lib().gpb_hip_vecchia_find_neighbors(self.h, C.byref(dup)))
        return bool(dup.value)

    def set_neighbors(self, nn):
        nn = np.ascontiguousarray(nn, dtype=np.int32)
        assert nn.shape == (self.n, self.m), (nn.shape, self.n, self.m)
        _shim_call(_lib().gpb_hip_vecchia_set_neighbors(self.h, _p(nn, C.c_int32)))

    def get_neighbors(self):
        nn = np.empty((self.n, self.m), dtype=np.int32)
        _shim_call(_lib().gpb_hip_vecchia_get_neighbors(self.h, _p(nn, C.c_int32)))
        return nn

    def set_shard(self, i_begin, i_end):
        _shim_call(_lib().gpb_hip_vecchia_set_shard(self.h, C.c_int(int(i_begin)), C.c_int(int(i_end))))

    def set_y(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        assert y.shape == (self.n,)
        _shim_call(_lib().gpb_hip_vecchia_set_y(self.h, _p(y)))

    def set_y_dev(self, y_dev_ptr):
        _shim_call(_lib().gpb_hip_vecchia_set_y_dev(self.h, C.c_void_p(int(y_dev_ptr))))

    def sync(self):
        _shim_call(_lib().gpb_hip_vecchia_sync(self.h))

    def nll_terms(self, cov_type, var, a, gauss=True):
        """-> array {y^T Psi^-1 y, log|Psi|, #bad} over this handle's shard."""
        out = np.empty(3)
        _shim_call(_lib().gpb_hip_vecchia_nll_terms(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a),
                                                    C.c_int(1 if gauss else 0), _p(out)))
        return out

    def nll_terms_dev(self, cov_type, var, a, out_dev_ptr, gauss=True):
        _shim_call(_lib().gpb_hip_vecchia_nll_terms_dev(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a),
                                                        C.c_int(1 if gauss else 0), C.c_void_p(int(out_dev_ptr))))

    def grad_terms(self, cov_type, var, a):
        out = np.empty(7)
        _shim_call(_lib().gpb_hip_vecchia_grad_terms(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(out)))
        return out

    def grad_terms_dev(self, cov_type, var, a, out_dev_ptr):
        _shim_call(_lib().gpb_hip_vecchia_grad_terms_dev(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a),
                                                         C.c_void_p(int(out_dev_ptr))))

    def comm_init(self, id128, rank, world):
        """Collective: bootstrap the in-library RCCL communicator from the 128-byte unique id of rank 0."""
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(id128))
        _shim_call(_lib().gpb_hip_vecchia_comm_init(self.h, buf, C.c_int(int(rank)), C.c_int(int(world))))

    def mailbox_attach(self, name, rank, world):
        """Collective: attach to the node-local shared-memory mailbox `name` (mailbox_create() on rank 0); the 3 / 7 sums of the sharded
        evaluations then travel through it instead of ncclAllReduce."""
        _shim_call(_lib().gpb_hip_vecchia_mailbox_attach(self.h, C.c_char_p(name if isinstance(name, bytes) else name.encode()), C.c_int(int(rank)), C.c_int(int(world))))

    def mailbox_info(self):
        r, w = C.c_int(0), C.c_int(0)
        _shim_call(_lib().gpb_hip_vecchia_mailbox_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def mailbox_detach(self):
        _shim_call(_lib().gpb_hip_vecchia_mailbox_detach(self.h))

    def timing(self, enable):
        """enable=True: record HIP events around every point-kernel launch; enable=False: -> (launches, mean kernel ms of the last <= 256)"""
        cnt = C.c_int64(0); ms = C.c_double(0.0)
        _shim_call(_lib().gpb_hip_vecchia_timing(self.h, C.c_int(1 if enable else 0), C.byref(cnt), C.byref(ms)))
        return cnt.value, ms.value

    def comm_init_local(self, group, rank):
        """Collective over the threads of an in-process group (LocalGroup) instead of RCCL."""
        _shim_call(_lib().gpb_hip_vecchia_comm_init_local(self.h, group.g, C.c_int(int(rank))))

    def comm_info(self):
        """(rank, number of ranks) as RCCL reports them for the handle's communicator (ncclCommUserRank / ncclCommCount); (0, 0) without one."""
        r, w = C.c_int(0), C.c_int(0)
        _shim_call(_lib().gpb_hip_vecchia_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def find_neighbors_part(self, part, nparts):
        dup = C.c_int(0)
        _shim_call(_lib().gpb_hip_vecchia_find_neighbors_part(self.h, C.c_int(int(part)), C.c_int(int(nparts)), C.byref(dup)))
        return bool(dup.value)

    def neighbors_allreduce(self):
        dup = C.c_int(0)
        _shim_call(_lib().gpb_hip_vecchia_neighbors_allreduce(self.h, C.byref(dup)))
        return bool(dup.value)

    def yaux_allreduce(self):
        out = np.empty(self.n)
        _shim_call(_lib().gpb_hip_vecchia_yaux_allreduce(self.h, _p(out)))
        return out

    def nll_terms_allreduce(self, cov_type, var, a, gauss=True):
        out = np.empty(3)
        _shim_call(_lib().gpb_hip_vecchia_nll_terms_allreduce(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a),
                                                              C.c_int(1 if gauss else 0), _p(out)))
        return out

    def grad_terms_allreduce(self, cov_type, var, a):
        out = np.empty(7)
        _shim_call(_lib().gpb_hip_vecchia_grad_terms_allreduce(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(out)))
        return out

    def bench(self, mode, cov_type, var, a, warmup, steps):
        """-> (ms_total, ms_point_kernel_avg, last_terms[7])"""
        t = C.c_double(0); k = C.c_double(0); out = np.empty(7)
        _shim_call(_lib().gpb_hip_vecchia_bench(self.h, C.c_int(mode), C.c_int(cov_type), C.c_double(var), C.c_double(a),
                                                C.c_int(warmup), C.c_int(steps), C.byref(t), C.byref(k), _p(out)))
        return t.value, k.value, out

    def factor(self, cov_type, var, a, gauss=True):
        _shim_call(_lib().gpb_hip_vecchia_factor(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a),
                                                 C.c_int(1 if gauss else 0)))

    def get_factor(self):
        A = np.empty((self.n, self.m)); D = np.empty(self.n); u = np.empty(self.n)
        _shim_call(_lib().gpb_hip_vecchia_get_factor(self.h, _p(A), _p(D), _p(u)))
        return A, D, u

    def yaux(self):
        out = np.empty(self.n)
        _shim_call(_lib().gpb_hip_vecchia_yaux(self.h, _p(out)))
        return out

    def predict_obs_only(self, coords_pred, num_neighbors_pred, cov_type, var, a):
        """-> (pred_mean, Dp, has_duplicates) for prediction points conditioning on the observed points only."""
        cp = np.asarray(coords_pred, dtype=np.float64)
        if cp.ndim == 1:
            cp = cp.reshape(-1, 1)
        cm = np.asfortranarray(cp)
        mu = np.empty(cp.shape[0]); Dp = np.empty(cp.shape[0]); dup = C.c_int(0)
        _shim_call(_lib().gpb_hip_vecchia_predict_obs_only(self.h, C.c_int(cp.shape[0]), _p(cm), C.c_int(int(num_neighbors_pred)),
                                                           C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(mu), _p(Dp), C.byref(dup)))
        return mu, Dp, bool(dup.value)

    def _pred_args(self, coords_pred, num_neighbors_pred, cond_all):
        """Column-major prediction coordinates and the number of table columns the C side will use (Vecchia_utils.cpp:755-758)."""
        cp = np.asarray(coords_pred, dtype=np.float64)
        if cp.ndim == 1:
            cp = cp.reshape(-1, 1)
        return np.asfortranarray(cp), cp.shape[0], min(int(num_neighbors_pred), self.n + cp.shape[0] - 1 if cond_all else self.n)

    def predict_cond_all(self, coords_pred, num_neighbors_pred, cov_type, var, a):
        """-> (nn_pred, A_pred, D_pred, has_duplicates): the factor rows of the appended prediction points, each conditioning on the observed
        AND the preceding prediction points; nn_pred indexes (observed, prediction), -1 padded."""
        cm, n_pred, m = self._pred_args(coords_pred, num_neighbors_pred, True)
        nn = np.empty((n_pred, m), dtype=np.int32); A = np.empty((n_pred, m)); D = np.empty(n_pred); dup = C.c_int(0); m_used = C.c_int32(0)
        _shim_call(_lib().gpb_hip_vecchia_predict_cond_all(self.h, C.c_int(n_pred), _p(cm), C.c_int(int(num_neighbors_pred)), C.c_int(cov_type), C.c_double(var),
                                                           C.c_double(a), C.byref(m_used), _p(nn, C.c_int32), _p(A), _p(D), C.byref(dup)))
        assert m_used.value == m, (m_used.value, m)
        return nn, A, D, bool(dup.value)

    def predict_joint_factor(self, coords_pred, num_neighbors_pred, layout_pred_first, cond_all, gauss, cov_type, var, a):
        """-> (nn_all, A_all, D_all, u_all, has_duplicates): the factor rows of EVERY point of the joint ordering, (observed, prediction) or --
        layout_pred_first -- (prediction, observed)."""
        cm, n_pred, m = self._pred_args(coords_pred, num_neighbors_pred, cond_all)
        n_all = self.n + n_pred
        nn = np.empty((n_all, m), dtype=np.int32); A = np.empty((n_all, m)); D = np.empty(n_all); u = np.empty(n_all); dup = C.c_int(0); m_used = C.c_int32(0)
        _shim_call(_lib().gpb_hip_vecchia_predict_joint_factor(self.h, C.c_int(n_pred), _p(cm), C.c_int(int(num_neighbors_pred)), C.c_int(1 if layout_pred_first else 0),
                                                               C.c_int(1 if cond_all else 0), C.c_int(1 if gauss else 0), C.c_int(cov_type), C.c_double(var), C.c_double(a),
                                                               C.byref(m_used), _p(nn, C.c_int32), _p(A), _p(D), _p(u), C.byref(dup)))
        assert m_used.value == m, (m_used.value, m)
        return nn, A, D, u, bool(dup.value)

    def newton_leaf_values(self, leaf_index, num_leaves):
        """Needs factor(gauss=True) and yaux() for the current y = F - y; leaf_index in Vecchia order."""
        leaf = np.ascontiguousarray(leaf_index, dtype=np.int32)
        out = np.empty(int(num_leaves))
        _shim_call(_lib().gpb_hip_vecchia_newton_leaf_values(self.h, _p(leaf, C.c_int), C.c_int(int(num_leaves)), _p(out)))
        return out

    def laplace_set_likelihood(self, likelihood):
        lid, self._lap_num_aux = _LIKELIHOODS[likelihood]
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_likelihood(self.h, C.c_int(lid)))

    def laplace_set_preconditioner(self, cg_preconditioner_type="vadu", rank=-999):
        """cg_preconditioner_type of the iterative methods: "vadu", "pivoted_cholesky" with `rank` columns, "fitc" with `rank` inducing points, or "vecchia_response"
        (evaluation only) -- gpb_hip_vecchia_laplace_set_preconditioner."""
        t = {"vadu": 0, "pivoted_cholesky": 1, "fitc": 2, "vecchia_response": 3, "vifdu": 4, "none": 5}[cg_preconditioner_type]      # (vifdu / none: full-scale Vecchia handles only)
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_preconditioner(self.h, C.c_int(t), C.c_int(int(rank))))

    def vif_set_inducing_points(self, ip):
        """Inducing points (k x d) of a full-scale Vecchia ("VIF") model (gpb_hip_vecchia_vif_set_inducing_points): the handle's Laplace evaluations then use
        Sigma = C Sigma_m^-1 C' + the Vecchia approximation of the residual process."""
        ipf = np.asfortranarray(ip, dtype=np.float64)
        _shim_call(_lib().gpb_hip_vecchia_vif_set_inducing_points(self.h, C.c_int(ipf.shape[0]), _p(ipf)))
        self._vif_k = ipf.shape[0]

    def _vif_kq(self):
        return (self._vif_k + 1 + 7) // 8 * 8

    def vif_factor(self, cov_type, var, a, Linv, with_grad=False):
        """gpb_hip_vecchia_vif_factor -> (out3 = {sum u^2 / D, sum log D, #(D <= 0)}, G (k + 1) x (k + 1)); Linv: k x k inverse Cholesky factor of Sigma_m."""
        Linv = np.ascontiguousarray(Linv, dtype=np.float64)
        k = Linv.shape[0]
        out3 = np.empty(3); G = np.empty((k + 1, k + 1))
        _shim_call(_lib().gpb_hip_vecchia_vif_factor(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(Linv), C.c_int(1 if with_grad else 0), _p(out3), _p(G)))
        return out3, G

    def vif_grad_sums(self, cov_type, var, a, Winv, Si, N0, negMp1, w, keep_factor=False):
        """gpb_hip_vecchia_vif_grad_sums -> sums12 in the order [2 * S + p]; the four matrices k x k (symmetric), w: k."""
        mats = [np.ascontiguousarray(M, dtype=np.float64) for M in (Winv, Si, N0, negMp1)]
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.empty(12)
        _shim_call(_lib().gpb_hip_vecchia_vif_grad_sums(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(mats[0]), _p(mats[1]), _p(mats[2]), _p(mats[3]),
                                                        _p(w), C.c_int(1 if keep_factor else 0), _p(out)))
        return out

    def vif_get_grad_factor(self, p):
        """dA (n x m), dD (n) of parameter p of the last vif_grad_sums(keep_factor = True)"""
        dA = np.empty((self.n, self.m)); dD = np.empty(self.n)
        _shim_call(_lib().gpb_hip_vecchia_vif_get_grad_factor(self.h, C.c_int(int(p)), _p(dA), _p(dD)))
        return dA, dD

    VIF_MATRICES = {"C": 0, "dC": 1, "V": 2, "Q": 3, "QdC": 4, "Hm": 5, "X1": 6, "V1": 7, "X2r": 8, "v": 9, "z": 10, "G": 11}      # GPB_VIF_MAT_* (include/gpb_hip.h)

    def vif_get_matrix(self, which):
        """Test seam (gpb_hip_vecchia_vif_get_matrix): a copy of one device buffer of the last vif_factor / vif_grad_sums: n x kq, or n (v, z), or kq x kq (G)."""
        kq = self._vif_kq()
        out = np.empty(self.n if which in ("v", "z") else ((kq, kq) if which == "G" else (self.n, kq)))
        _shim_call(_lib().gpb_hip_vecchia_vif_get_matrix(self.h, C.c_int(self.VIF_MATRICES[which]), _p(out)))
        return out

    def vif_get_point_terms(self, nterms):
        """Test seam (gpb_hip_vecchia_vif_get_point_terms): the per-point partials [nterms][n], 3 after vif_factor, 12 after vif_grad_sums."""
        out = np.empty((int(nterms), self.n))
        _shim_call(_lib().gpb_hip_vecchia_vif_get_point_terms(self.h, C.c_int(int(nterms)), _p(out)))
        return out

    def laplace_set_inducing_points(self, ip):
        """Inducing points (k x d) of the "fitc" preconditioner (gpb_hip_vecchia_laplace_set_inducing_points)."""
        ipf = np.asfortranarray(ip, dtype=np.float64)
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_inducing_points(self.h, C.c_int(ipf.shape[0]), _p(ipf)))

    def laplace_set_response_real(self, y):
        """gamma: the real-valued response (> 0), in the order laplace_set_labels takes its labels."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_response_real(self.h, _p(y)))

    def set_sorted_gather(self, mode):
        """-1: default (n >= 32768, from the third evaluation), 0: never, 1: always -- the spatially sorted copy of the records the neighbour gathers read."""
        _shim_call(_lib().gpb_hip_vecchia_set_sorted_gather(self.h, C.c_int(int(mode))))

    def set_nugget_diag(self, nug):
        """Sample weights of the Gaussian likelihood: nug[i] = 1 / w_i in Vecchia order, the diagonals become var + nug[.] (gpb_hip_vecchia_set_nugget_diag);
        None goes back to the uniform nugget."""
        if nug is not None:
            nug = np.ascontiguousarray(nug, dtype=np.float64)
            assert nug.shape == (self.n,)
        _shim_call(_lib().gpb_hip_vecchia_set_nugget_diag(self.h, _p(nug)))

    def set_worker_cap(self, cap):
        """Test seam: at most `cap` persistent workers per point-kernel launch, 0 = the default grid (gpb_hip_vecchia_set_worker_cap)."""
        _shim_call(_lib().gpb_hip_vecchia_set_worker_cap(self.h, C.c_int(int(cap))))

    def laplace_set_weights(self, w):
        """Sample weights of the non-Gaussian likelihood, in the order of the labels (gpb_hip_vecchia_laplace_set_weights); None removes them."""
        ww = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_weights(self.h, _p(ww)))

    def laplace_set_binomial(self, on=True):
        """binomial_logit / binomial_probit: the binomial normalising constant over (proportions, trials = sample weights) (gpb_hip_vecchia_laplace_set_binomial)."""
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_binomial(self.h, C.c_int(int(bool(on)))))

    def laplace_set_aux(self, aux):
        """gamma / negative_binomial: the shape parameter (gpb_hip_vecchia_laplace_set_aux_pars)."""
        a = np.ascontiguousarray(np.atleast_1d(aux), dtype=np.float64)
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_aux_pars(self.h, _p(a), C.c_int(a.size)))

    def laplace_grad_aux(self):
        """-> {gradient wrt log(shape), CalcGradNegLogLikAuxPars part, log-determinant part, implicit part} at the state of the last laplace_eval_grad."""
        o = np.zeros(8)          # 4 per auxiliary parameter (t has two: scale, df)
        _shim_call(_lib().gpb_hip_vecchia_laplace_grad_aux_current(self.h, _p(o)))
        return o if getattr(self, "_lap_num_aux", 0) == 2 else o[:4]

    def laplace_set_fixed_effects(self, fixed_effects):
        """Offset of the location parameter, Vecchia order (None removes it)."""
        fe = None if fixed_effects is None else np.ascontiguousarray(fixed_effects, dtype=np.float64)
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_fixed_effects(self.h, _p(fe)))

    def laplace_set_labels(self, y01):
        y01 = np.ascontiguousarray(y01, dtype=np.int32)
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_labels(self.h, _p(y01, C.c_int)))

    def laplace_logit(self, cov_type, var, a, num_rand_vec=50, seed_rand_vec=1, cg_max_num_it=1000, cg_max_num_it_tridiag=1000,
                      cg_delta_conv=1e-2, delta_conv_mode_finding=1e-8, reset_mode=True, want_mode=False):
        """-> (negll, info): Vecchia-Laplace approximation, Bernoulli-logit, iterative methods (gpb_hip_vecchia_laplace_logit)."""
        o = np.empty(9)
        mode = np.empty(self.n) if want_mode else None
        _shim_call(_lib().gpb_hip_vecchia_laplace_logit(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), C.c_int(num_rand_vec),
                                                        C.c_int(seed_rand_vec), C.c_int(cg_max_num_it), C.c_int(cg_max_num_it_tridiag),
                                                        C.c_double(cg_delta_conv), C.c_double(delta_conv_mode_finding),
                                                        C.c_int(1 if reset_mode else 0), _p(o), _p(mode)))
        return -o[0], dict(newton_it=int(o[1]), cg_it=int(o[2]), log_det=o[3], lanczos_it=int(o[4]), mll_no_det=o[5],
                           ms_factor=o[6], ms_mode=o[7], ms_logdet=o[8], mode=mode)

    def laplace_eval_grad(self, cov_type, var, a, num_rand_vec=50, seed_rand_vec=1, cg_max_num_it=1000, cg_max_num_it_tridiag=1000,
                          cg_delta_conv=1e-2, delta_conv_mode_finding=1e-8, reset_mode=True, want_parts=False):
        """-> (negll, grad wrt (log var, log a)[, parts]): Vecchia-Laplace approximation and its gradient on the device
        (gpb_hip_vecchia_laplace_eval + gpb_hip_vecchia_laplace_grad_current)."""
        o = np.empty(9)
        _shim_call(_lib().gpb_hip_vecchia_laplace_eval(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), C.c_int(num_rand_vec),
                                                       C.c_int(seed_rand_vec), C.c_int(cg_max_num_it), C.c_int(cg_max_num_it_tridiag),
                                                       C.c_double(cg_delta_conv), C.c_double(delta_conv_mode_finding),
                                                       C.c_int(1 if reset_mode else 0), C.c_int(1), _p(o), None))
        g = np.empty(2)
        parts = np.empty(8) if want_parts else None
        vecs = np.empty(2 * self.n) if want_parts else None
        _shim_call(_lib().gpb_hip_vecchia_laplace_grad_current(self.h, C.c_int(cg_max_num_it), C.c_double(cg_delta_conv), _p(g), _p(parts), _p(vecs)))
        if getattr(self, "_lap_num_aux", 0) == 2:      # t: d / d (log scale, log df)
            ga = self.laplace_grad_aux()
            g = np.array([g[0], g[1], ga[0], ga[4]])
        elif getattr(self, "_lap_num_aux", 0) == 1:      # likelihoods with one auxiliary parameter: third entry = d / d log(aux)
            g = np.array([g[0], g[1], self.laplace_grad_aux()[0]])
        if want_parts:
            return -o[0], g, dict(per_par=parts.reshape(2, 4), dlogdet_dmode=vecs[:self.n], implicit_solve=vecs[self.n:])
        return -o[0], g

    def laplace_set_data_map(self, re_ptr):
        """Repeated locations: the state's n points are the unique locations, re_ptr (n + 1) the CSR of their data; labels / fixed effects are
        then handed over grouped by random effect (gpb_hip_vecchia_laplace_set_data_map).  None: one datum per random effect."""
        rp = None if re_ptr is None else np.ascontiguousarray(re_ptr, dtype=np.int32)
        self._n_data = self.n if rp is None else int(rp[-1])
        _shim_call(_lib().gpb_hip_vecchia_laplace_set_data_map(self.h, _p(rp, C.c_int)))

    def laplace_grad_F(self):
        """Boosting gradient d(-mll)/dF at the state of the last laplace_eval_grad (gpb_hip_vecchia_laplace_grad_F_current): Vecchia order, or --
        with a data map -- per datum in the grouped order of the labels."""
        out = np.empty(getattr(self, "_n_data", self.n))
        _shim_call(_lib().gpb_hip_vecchia_laplace_grad_F_current(self.h, _p(out)))
        return out

    def laplace_reset_mode_to_previous(self):
        _shim_call(_lib().gpb_hip_vecchia_laplace_reset_mode_to_previous(self.h))

    def laplace_range_deriv(self, cov_type, var, a):
        """-> (dA / d log a [n, m], dD / d log a [n]) of the factor without nugget (test seam, gpb_hip_vecchia_laplace_range_deriv)."""
        dA = np.empty((self.n, self.m)); dD = np.empty(self.n)
        _shim_call(_lib().gpb_hip_vecchia_laplace_range_deriv(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(dA), _p(dD)))
        return dA, dD

    _LAP_OPS = {"B": 0, "Bt": 1, "apply": 2, "vadu": 3, "fwd_solve": 4, "mul_fwd": 5, "mul_bwd": 6}
    _LAP_PREFILL = {"zeros": 0, "nan": 1, "inf": 2, "sentinel": 3}
    _LAP_INFO = ("nlev", "nslots", "novf", "dense_K", "wide_segments", "run_segments", "padding_slots", "split_rows", "long_slots")

    def laplace_ops_check(self, op, A, X, nc=1, form=0, prefill="zeros", D=None, W=None, scale=None, A2=None):
        """One launcher of the sparse Vecchia-Laplace machinery on the caller's factor (gpb_hip_vecchia_laplace_ops_check; test seam).  A (n, m), D / W / scale (n)
        and the columns X (n, ncol * nc) in Vecchia order; form 0 = one launch per level, 1 / 4 = barrier-free (single vectors / probe block); prefill: what the results
        and the scratch hold before the launch.  -> (out, out2 or None, info): results (n, ncol * nc), out2 = D^-1 B X of "apply" / t of "vadu"; info: dict with "fwd" and
        "bwd" (the schedule's counts, _LAP_INFO), "err" (error word of the solves), "resident" (single vectors, probe block)."""
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        A = f64(A); X = np.asarray(X, dtype=np.float64)
        Dc, Wc, Sc, A2c = f64(D), f64(W), f64(scale), f64(A2)
        assert A.shape == (self.n, self.m) and X.ndim == 2 and X.shape[0] == self.n and X.shape[1] % nc == 0, (A.shape, X.shape, nc)
        Xc = np.ascontiguousarray(X.T)
        out = np.empty_like(Xc)
        opi = self._LAP_OPS[op]
        out2 = np.empty_like(Xc) if opi in (2, 3) else None
        info = np.zeros(24, dtype=np.int32)
        for v in (D, W, scale):
            assert v is None or np.shape(v) == (self.n,)
        assert A2 is None or np.shape(A2) == A.shape
        _shim_call(_lib().gpb_hip_vecchia_laplace_ops_check(self.h, C.c_int(opi), C.c_int(int(form)), C.c_int(X.shape[1] // nc), C.c_int(int(nc)),
                                                            C.c_int(self._LAP_PREFILL[prefill]), _p(A), _p(Dc), _p(Wc), _p(Sc), _p(A2c), _p(Xc),
                                                            _p(out), _p(out2), _p(info, C.c_int32)))
        d = {"fwd": dict(zip(self._LAP_INFO, (int(v) for v in info[:9]))), "bwd": dict(zip(self._LAP_INFO, (int(v) for v in info[9:18]))),
             "err": int(info[18]), "resident": (int(info[19]), int(info[20]))}
        return out.T, (None if out2 is None else out2.T), d

    def yaux_partial_dev(self, w_dev_ptr):
        """This shard's contribution to y_aux as a full n-vector on the device (sum over ranks = y_aux)."""
        _shim_call(_lib().gpb_hip_vecchia_yaux_partial_dev(self.h, C.c_void_p(int(w_dev_ptr))))


class DeviceBuffer(object):
    """n doubles of device memory (gpb_hip_dev_alloc); .ptr is what the *_dev entry points take."""

    def __init__(self, n):
        self.n = int(n)
        self.p = C.c_void_p()
        _shim_call(_lib().gpb_hip_dev_alloc(C.c_uint64(8 * self.n), C.byref(self.p)))

    @property
    def ptr(self):
        return self.p.value

    def to_host(self):
        out = np.empty(self.n)
        _shim_call(_lib().gpb_hip_dev_to_host(_p(out), self.p, C.c_uint64(8 * self.n)))
        return out

    def from_host(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.size != self.n:
            raise ValueError("values must have %d entries" % self.n)
        _shim_call(_lib().gpb_hip_dev_from_host(self.p, _p(v), C.c_uint64(8 * self.n)))
        return self

    def __del__(self):
        try:
            if self.p.value:
                _lib().gpb_hip_dev_free(self.p)
                self.p = C.c_void_p()
        except Exception:
            pass


class ExactState(object):
    """Exact (dense) GP: coords (n, d) in data order."""

    def __init__(self, coords):
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim == 1:
            coords = coords.reshape(-1, 1)
        self.n, self.d = coords.shape
        cm = np.asfortranarray(coords)
        self.h = C.c_void_p()
        _shim_call(_lib().gpb_hip_exact_create(C.c_int(self.n), C.c_int(self.d), _p(cm), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value is not None:
            _lib().gpb_hip_exact_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_y(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        assert y.shape == (self.n,)
        _shim_call(_lib().gpb_hip_exact_set_y(self.h, _p(y)))

    def nll_terms(self, cov_type, var, a, want_yaux=False):
        """-> (array {y^T Psi^-1 y, log|Psi|}, yaux or None, ms {assembly, factorisation, solves})"""
        out = np.empty(2); ms = np.empty(3)
        ya = np.empty(self.n) if want_yaux else None
        _shim_call(_lib().gpb_hip_exact_nll_terms(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(out),
                                                  _p(ya), _p(ms)))
        return out, ya, ms

    def grad_terms(self, cov_type, var, a):
        """-> array {y' Psi^-1 y, log|Psi|, 0, g1_var, g2_var, g1_range, g2_range} (gpb_hip_exact_grad_terms)"""
        out = np.empty(7)
        _shim_call(_lib().gpb_hip_exact_grad_terms(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(out)))
        return out

    def psi_inv_diag(self, cov_type, var, a):
        """-> diag(Psi^-1), n entries (gpb_hip_exact_psi_inv_diag)"""
        out = np.empty(self.n)
        _shim_call(_lib().gpb_hip_exact_psi_inv_diag(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), _p(out)))
        return out

    def predict(self, coords_pred, want_q, cov_type, var, a):
        """coords_pred (n_pred, d) -> (C Psi^-1 y, C Psi^-1 C' (n_pred, n_pred) or None) on the transformed scale (gpb_hip_exact_predict)"""
        cp = np.asarray(coords_pred, dtype=np.float64)
        if cp.ndim == 1:
            cp = cp.reshape(-1, 1)
        assert cp.shape[1] == self.d
        npred = cp.shape[0]
        cm = np.asfortranarray(cp)
        mean = np.empty(npred)
        q = np.empty((npred, npred)) if want_q else None
        _shim_call(_lib().gpb_hip_exact_predict(self.h, C.c_int(cov_type), C.c_double(var), C.c_double(a), C.c_int(npred), _p(cm), _p(mean), _p(q)))
        return mean, q


def dense_cholesky_check(M, ncols=None, lookahead=False):
    """The blocked Cholesky on the (ld, ld) matrix M, ld a multiple of 64, first ncols columns (gpb_hip_dense_cholesky_check).
    -> (out, info): L, the Schur complement and the untouched strict upper triangle; info != 0 if a pivot was not positive."""
    M = np.ascontiguousarray(M, dtype=np.float64)
    ld = M.shape[0]
    assert M.shape == (ld, ld)
    out = np.empty_like(M)
    info = C.c_int32(-1)
    _shim_call(_lib().gpb_hip_dense_cholesky_check(C.c_int(ld), C.c_int(ld if ncols is None else int(ncols)), C.c_int(1 if lookahead else 0), _p(M), _p(out),
                                                   C.byref(info)))
    return out, int(info.value)


def dense_spd_solve(M, rhs=None, sub0=None):
    """M (n, n) symmetric positive definite, lower triangle significant (gpb_hip_dense_spd_solve).  -> (x = M^-1 rhs or None, rows / columns [sub0, n) of M^-1 or None)"""
    M = np.ascontiguousarray(M, dtype=np.float64)
    n = M.shape[0]
    assert M.shape == (n, n)
    r = None if rhs is None else np.ascontiguousarray(rhs, dtype=np.float64)
    assert r is None or r.shape == (n,)
    x = None if r is None else np.empty(n)
    inv = None if sub0 is None else np.empty((n - int(sub0), n - int(sub0)))
    _shim_call(_lib().gpb_hip_dense_spd_solve(C.c_int(n), _p(M), _p(r), _p(x), C.c_int(0 if sub0 is None else int(sub0)), _p(inv)))
    return x, inv


def laplace_lik_check(lik, mode, D, dld, sv, y_int=None, y_real=None, re_ptr=None, weights=None, fixed_effects=None, Bx=None, aux=1.0, aux2=2.0, n_each=0):
    """The likelihood kernels of the Vecchia-Laplace path on the caller's data (gpb_hip_laplace_lik_check, op 0; test seam).  lik: a name of _LIKELIHOODS or an id;
    mode, D, dld, sv (n) and Bx (n) or None; re_ptr (n + 1) or None; exactly one of y_int / y_real, weights and fixed_effects per datum.
    -> dict: W, rhs, dw, rdw, dW3 (n), out2 (2), ll_each (n_each), gradF (n, or n_data with re_ptr), out3 (3)"""
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    lid = _LIKELIHOODS[lik][0] if isinstance(lik, str) else int(lik)
    mode, D, dld, sv, Bx, w, fe, yr = f64(mode), f64(D), f64(dld), f64(sv), f64(Bx), f64(weights), f64(fixed_effects), f64(y_real)
    yi, ptr = i32(y_int), i32(re_ptr)
    n = mode.shape[0]
    assert (yi is None) != (yr is None)
    n_data = (yi if yr is None else yr).shape[0]
    assert ptr is None or ptr.shape == (n + 1,)
    for v in (D, dld, sv, Bx):
        assert v is None or v.shape == (n,)
    for v in (w, fe):
        assert v is None or v.shape == (n_data,)
    r = {k: np.empty(n) for k in ("W", "rhs", "dw", "rdw", "dW3")}
    r.update(out2=np.empty(2), ll_each=np.empty(int(n_each)), gradF=np.empty(n_data), out3=np.empty(3))
    _shim_call(_lib().gpb_hip_laplace_lik_check(C.c_int(0), C.c_int(lid), C.c_int(n), C.c_int(n_data), _p(ptr, C.c_int32), _p(yi, C.c_int32), _p(yr), _p(w), _p(fe),
                                                _p(mode), _p(D), _p(Bx), _p(dld), _p(sv), C.c_double(aux), C.c_double(aux2), C.c_int(int(n_each)), _p(r["W"]),
                                                _p(r["rhs"]), _p(r["dw"]), _p(r["rdw"]), _p(r["out2"]), _p(r["ll_each"]), _p(r["dW3"]), _p(r["gradF"]), _p(r["out3"])))
    return r


_MATH_PROBE_FNS = ("exp", "log", "log1p", "erfc", "lgamma", "sqrt")


def math_probe(fn, x):
    """The device's library function fn (one of _MATH_PROBE_FNS) on the vector x, compiled as the likelihood kernels are (gpb_hip_laplace_lik_check, op 1; test seam)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    nul = C.POINTER(C.c_double)()
    _shim_call(_lib().gpb_hip_laplace_lik_check(C.c_int(1), C.c_int(_MATH_PROBE_FNS.index(fn)), C.c_int(x.shape[0]), C.c_int(x.shape[0]), None, None, nul, nul, nul,
                                                _p(x), nul, nul, nul, nul, C.c_double(0.0), C.c_double(0.0), C.c_int(0), _p(out), nul, nul, nul, nul, nul, nul, nul, nul))
    return out


class LocalGroup(object):
    """In-process group of `world` ranks (threads of this process; their handles may share one device): the second transport behind the
    library's collectives (gpb_hip_local_group_create).  `run(fn)` calls fn(rank) on one thread per rank and returns the results in rank
    order; an exception on any rank aborts the group so that no peer waits in a barrier for ever."""

    def __init__(self, world):
        self.world = int(world)
        self.g = C.c_void_p()
        _shim_call(_lib().gpb_hip_local_group_create(C.c_int(self.world), C.byref(self.g)))

    def close(self):
        if getattr(self, "g", None) is not None and self.g.value is not None:
            _lib().gpb_hip_local_group_free(self.g)
            self.g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def abort(self):
        _lib().gpb_hip_local_group_abort(self.g)

    def run(self, fn):
        import threading
        res, err = [None] * self.world, [None] * self.world

        def work(r):
            try:
                res[r] = fn(r)
            except BaseException as e:        # noqa: BLE001 -- re-raised on the calling thread
                err[r] = e
                self.abort()
        th = [threading.Thread(target=work, args=(r,)) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for e in err:
            if e is not None:
                raise e
        return res


def lowrank_ops_check(op, L, W, ncol=1, nc=4, M=None, X=None, x2=None, mode=0, in_place=False, guard=64, sentinel=-7.25e300):
    """One block operation of the low-rank preconditioners on the device (gpb_hip_lowrank_ops_check; layouts: csrc/pivchol_kernels.h).  op "gram": L' diag(W) L, packed
    lower triangle; "ltwx": M (L' (W .* X)) -> (ncol, k, nc); "combine": modes 0..4 on X (ncol, n, nc) and x2 (ncol, k, nc) -> (ncol, n, nc), in_place: out == X on the device.
    -> (result, guards_intact): the result lies between two runs of `guard` sentinels on the device; guards_intact tells that both came back unchanged."""
    L = np.ascontiguousarray(L, dtype=np.float64); W = np.ascontiguousarray(W, dtype=np.float64)
    n, k = L.shape
    opi = {"gram": 0, "ltwx": 1, "combine": 2}[op]
    shape = (k * (k + 1) // 2,) if opi == 0 else ((ncol, k, nc) if opi == 1 else (ncol, n, nc))
    size = int(np.prod(shape))
    Mc = None if M is None else np.ascontiguousarray(M, dtype=np.float64)
    Xc = None if X is None else np.ascontiguousarray(X, dtype=np.float64)
    x2c = None if x2 is None else np.ascontiguousarray(x2, dtype=np.float64)
    assert W.shape == (n,) and (Mc is None or Mc.shape == (k, k)) and (Xc is None or Xc.shape == (ncol, n, nc)) and (x2c is None or x2c.shape == (ncol, k, nc))
    out = np.full(size + 2 * guard, sentinel)
    if opi == 2 and in_place:
        out[guard:guard + size] = Xc.ravel()
    _shim_call(_lib().gpb_hip_lowrank_ops_check(C.c_int(opi), C.c_int(n), C.c_int(k), C.c_int(ncol), C.c_int(nc), C.c_int(mode), _p(L), _p(W), _p(Mc), _p(Xc), _p(x2c),
                                                C.c_int(1 if in_place else 0), C.c_int(guard), _p(out)))
    intact = bool(np.all(out[:guard] == sentinel) and np.all(out[guard + size:] == sentinel))
    return out[guard:guard + size].reshape(shape).copy(), intact


def mailbox_create(world):
    """rank 0: create the node-local mailbox segment for `world` ranks -> its name (bytes; hand it to every rank's mailbox_attach)"""
    buf = C.create_string_buffer(64)
    _shim_call(_lib().gpb_hip_mailbox_create(C.c_int(int(world)), buf))
    return buf.value


def comm_unique_id():
    """128-byte ncclUniqueId (call on rank 0, broadcast to the other ranks)."""
    buf = (C.c_ubyte * 128)()
    _shim_call(_lib().gpb_hip_comm_get_unique_id(buf))
    return bytes(buf)


def nll_from_terms(n, yPy, logdet, sigma2):
    """include/GPBoost/re_model_template.h:3132"""
    return yPy / 2. / sigma2 + logdet / 2. + n / 2. * (np.log(sigma2) + np.log(2 * np.pi))


def grad_from_terms(n, t7, sigma2):
    """include/GPBoost/re_model_template.h:1994,2004 -> d nll / d log(sigma2, var, a)"""
    return np.array([-t7[0] / sigma2 / 2. + n / 2., t7[3] / sigma2 + t7[4], t7[5] / sigma2 + t7[6]])


class HistBuilder(object):
    """bins: (F, n) uint8 feature-major; bin_offsets: F+1 prefix sums."""

    def __init__(self, bins, bin_offsets):
        bins = np.ascontiguousarray(bins, dtype=np.uint8)
        self.F, self.n = bins.shape
        self.bin_offsets = np.ascontiguousarray(bin_offsets, dtype=np.int32)
        self.total_bins = int(self.bin_offsets[-1])
        self.h = C.c_void_p()
        _shim_call(_lib().gpb_hip_hist_create(C.c_int(self.n), C.c_int(self.F), _p(bins, C.c_uint8),
                                              _p(self.bin_offsets, C.c_int32), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value is not None:
            _lib().gpb_hip_hist_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_gradients(self, grad, hess=None):
        grad = np.ascontiguousarray(grad, dtype=np.float64)
        hess = None if hess is None else np.ascontiguousarray(hess, dtype=np.float64)
        _shim_call(_lib().gpb_hip_hist_set_gradients(self.h, _p(grad), _p(hess)))

    def bench(self, data_indices=None, const_hess=1.0, reps=10):
        """mean ms of one leaf build (kernels only, HIP events)"""
        di = None if data_indices is None else np.ascontiguousarray(data_indices, dtype=np.int32)
        nd = self.n if di is None else di.size
        ms = C.c_double(0)
        _shim_call(_lib().gpb_hip_hist_bench(self.h, _p(di, C.c_int32), C.c_int(nd), C.c_double(const_hess), C.c_int(reps),
                                             C.byref(ms)))
        return ms.value

    def comm_init(self, id128, rank, world):
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(id128))
        _shim_call(_lib().gpb_hip_hist_comm_init(self.h, buf, C.c_int(int(rank)), C.c_int(int(world))))

    def comm_init_local(self, group, rank):
        _shim_call(_lib().gpb_hip_hist_comm_init_local(self.h, group.g, C.c_int(int(rank))))

    def build_allreduce(self, data_indices=None, const_hess=1.0):
        """Local leaf histogram of this rank's rows + all-reduce over the ranks -> (hist (total_bins, 2), cnt)."""
        idx = None if data_indices is None else np.ascontiguousarray(data_indices, dtype=np.int32)
        nd = self.n if idx is None else idx.size
        hist = np.empty((self.total_bins, 2)); cnt = np.empty(self.total_bins, dtype=np.uint64)
        _shim_call(_lib().gpb_hip_hist_build_allreduce(self.h, _p(idx, C.c_int), C.c_int(nd), C.c_double(const_hess), _p(hist),
                                                       _p(cnt, C.c_uint64)))
        return hist, cnt

    # ---- resident leaf histograms (row a12) ----
    def pool_resize(self, num_slots):
        _shim_call(_lib().gpb_hip_hist_pool_resize(self.h, C.c_int(int(num_slots))))

    def set_fix_info(self, view_offset, num_bin, most_freq_bin):
        vo = np.ascontiguousarray(view_offset, dtype=np.int32); nb = np.ascontiguousarray(num_bin, dtype=np.int32)
        mf = np.ascontiguousarray(most_freq_bin, dtype=np.int32)
        _shim_call(_lib().gpb_hip_hist_set_fix_info(self.h, _p(vo, C.c_int), _p(nb, C.c_int), _p(mf, C.c_int)))

    def build_slot(self, slot, data_indices=None, const_hess=1.0):
        idx = None if data_indices is None else np.ascontiguousarray(data_indices, dtype=np.int32)
        nd = self.n if idx is None else idx.size
        _shim_call(_lib().gpb_hip_hist_build_slot(self.h, C.c_int(int(slot)), _p(idx, C.c_int), C.c_int(nd), C.c_double(const_hess)))

    def fix_slot(self, slot, sum_gradient, sum_hessian):
        _shim_call(_lib().gpb_hip_hist_fix_slot(self.h, C.c_int(int(slot)), C.c_double(sum_gradient), C.c_double(sum_hessian)))

    def subtract_slots(self, parent, smaller, out):
        _shim_call(_lib().gpb_hip_hist_subtract_slots(self.h, C.c_int(int(parent)), C.c_int(int(smaller)), C.c_int(int(out))))

    def set_split_info(self, offset, default_bin, missing_type):
        a = [np.ascontiguousarray(x, dtype=np.int32) for x in (offset, default_bin, missing_type)]
        _shim_call(_lib().gpb_hip_hist_set_split_info(self.h, *[_p(x, C.c_int) for x in a]))

    def set_categorical(self, is_categorical, max_cat_to_onehot=4, max_cat_threshold=32, cat_smooth=10.0, cat_l2=10.0, min_data_per_group=100):
        """Categorical features: flags per feature (None: all numerical) and the reference's Config values of the same names
        (FindBestThresholdCategoricalInner, feature_histogram.hpp:278-519); they stay set for find_best_split and grow_tree."""
        m = None if is_categorical is None else np.ascontiguousarray(np.asarray(is_categorical) != 0, dtype=np.int8)
        if m is not None and m.size != self.F:
            raise ValueError("is_categorical must have one flag per feature")
        self.is_categorical = np.zeros(self.F, dtype=np.int8) if m is None else m
        _shim_call(_lib().gpb_hip_hist_set_categorical(self.h, _p(m, C.c_int8), C.c_int(int(max_cat_to_onehot)), C.c_int(int(max_cat_threshold)),
                                                       C.c_double(cat_smooth), C.c_double(cat_l2), C.c_int(int(min_data_per_group))))

    def set_feature_block_exchange(self, on=True):
        """Data-parallel tree grower: reduce-scatter by feature block + exchange of the ranks' best splits (default) or all-reduce of every histogram."""
        _shim_call(_lib().gpb_hip_hist_set_feature_block_exchange(self.h, C.c_int(-1 if on is None else int(bool(on)))))

    def set_regularisation(self, lambda_l1=0.0, max_delta_step=0.0, path_smooth=0.0, parent_output=0.0):
        """lambda_l1 / max_delta_step / path_smooth of the split search (they stay set for find_best_split and grow_tree); parent_output: the
        leaf's own output, for the following find_best_split calls (path smoothing; grow_tree tracks it itself)."""
        _shim_call(_lib().gpb_hip_hist_set_regularisation(self.h, C.c_double(lambda_l1), C.c_double(max_delta_step), C.c_double(path_smooth),
                                                          C.c_double(parent_output)))

    def set_root_rows(self, rows=None):
        """Bagging: the (ascending) rows the root of the following trees holds; None = all rows."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        _shim_call(_lib().gpb_hip_hist_set_root_rows(self.h, _p(r, C.c_int), C.c_int(0 if r is None else r.size)))

    def set_feature_mask(self, is_feature_used=None):
        """The columns grow_tree may split on (feature_fraction's per-tree sample); None = all."""
        m = None if is_feature_used is None else np.ascontiguousarray(is_feature_used, dtype=np.int8)
        if m is not None and m.size != self.F:
            raise ValueError("is_feature_used must have one flag per feature")
        _shim_call(_lib().gpb_hip_hist_set_feature_mask(self.h, _p(m, C.c_int8)))

    def set_max_depth(self, max_depth):
        """config max_depth of grow_tree (<= 0: no limit)."""
        _shim_call(_lib().gpb_hip_hist_set_max_depth(self.h, C.c_int(int(max_depth))))

    def find_best_split(self, slot, sum_gradient, sum_hessian, num_data, lambda_l2=0.0, min_data_in_leaf=20,
                        min_sum_hessian_in_leaf=1e-3, min_gain_to_split=0.0, is_feature_used=None):
        """-> (best_feature, out (F, 10), default_left (F,)): FeatureHistogram::FindBestThreshold per feature + the winner;
        self.last_splittable holds is_splittable() per feature."""
        out = np.empty((self.F, 10)); dl = np.empty(self.F, dtype=np.int32); best = C.c_int(-1)
        self.last_splittable = np.empty(self.F, dtype=np.int32)
        used = None if is_feature_used is None else np.ascontiguousarray(is_feature_used, dtype=np.int8)
        _shim_call(_lib().gpb_hip_hist_find_best_split(self.h, C.c_int(int(slot)), C.c_double(sum_gradient), C.c_double(sum_hessian),
                                                       C.c_int(int(num_data)), C.c_double(lambda_l2), C.c_int(int(min_data_in_leaf)),
                                                       C.c_double(min_sum_hessian_in_leaf), C.c_double(min_gain_to_split),
                                                       _p(used, C.c_int8), C.byref(best), _p(out), _p(dl, C.c_int),
                                                       _p(self.last_splittable, C.c_int)))
        # categorical features: the sets of bins going left (8 words per feature; zeros for numerical features)
        self.last_cat_bits = np.zeros((self.F, 8), dtype=np.uint32)
        _shim_call(_lib().gpb_hip_hist_last_split_cat_bits(self.h, _p(self.last_cat_bits, C.c_uint32)))
        return best.value, out, dl

    def split_leaf(self, data_indices, feature, threshold, default_left, cat_bits=None):
        """-> (lte_indices, gt_indices), both in the order of data_indices (None = all rows).  cat_bits (8 words): a categorical split, the rows whose
        bin is in the set go left."""
        idx = None if data_indices is None else np.ascontiguousarray(data_indices, dtype=np.int32)
        cnt = self.n if idx is None else idx.size
        lte = np.empty(cnt, dtype=np.int32); gt = np.empty(cnt, dtype=np.int32); nl = C.c_int(0)
        if cat_bits is not None:
            w = np.ascontiguousarray(cat_bits, dtype=np.uint32)
            _shim_call(_lib().gpb_hip_hist_split_leaf_categorical(self.h, _p(idx, C.c_int), C.c_int(cnt), C.c_int(int(feature)), _p(w, C.c_uint32),
                                                                  _p(lte, C.c_int), _p(gt, C.c_int), C.byref(nl)))
            return lte[:nl.value].copy(), gt[:cnt - nl.value].copy()
        _shim_call(_lib().gpb_hip_hist_split_leaf(self.h, _p(idx, C.c_int), C.c_int(cnt), C.c_int(int(feature)), C.c_uint(int(threshold)),
                                                  C.c_int(int(bool(default_left))), _p(lte, C.c_int), _p(gt, C.c_int), C.byref(nl)))
        return lte[:nl.value].copy(), gt[:cnt - nl.value].copy()

    def grow_tree(self, num_leaves, sum_gradient, sum_hessian, lambda_l2=0.0, min_data_in_leaf=20, min_sum_hessian_in_leaf=1e-3,
                  min_gain_to_split=0.0, const_hess=1.0, want_leaf_index=True):
        """One leaf-wise tree with device-resident row lists (gpb_hip_hist_grow_tree).  Returns the arrays of tests/tree_harness.grow_tree
        plus 'data_leaf_index'."""
        L = int(num_leaves)
        nl = C.c_int(0)
        ia = {k: np.zeros(L, dtype=np.int32) for k in ("split_feature_inner", "default_left", "left_child", "right_child", "internal_count", "leaf_count")}
        thr = np.zeros(L, dtype=np.uint32); gain = np.zeros(L); lv = np.zeros(L)
        dli = np.empty(self.n, dtype=np.int32) if want_leaf_index else None
        _shim_call(_lib().gpb_hip_hist_grow_tree(
            self.h, C.c_int(L), C.c_double(sum_gradient), C.c_double(sum_hessian), C.c_double(lambda_l2), C.c_int(int(min_data_in_leaf)),
            C.c_double(min_sum_hessian_in_leaf), C.c_double(min_gain_to_split), C.c_double(const_hess), C.byref(nl),
            _p(ia["split_feature_inner"], C.c_int), _p(thr, C.c_uint32), _p(ia["default_left"], C.c_int), _p(ia["left_child"], C.c_int),
            _p(ia["right_child"], C.c_int), _p(gain), _p(ia["internal_count"], C.c_int), _p(lv), _p(ia["leaf_count"], C.c_int),
            None if dli is None else _p(dli, C.c_int)))
        k = nl.value
        out = dict(num_leaves=k, threshold_in_bin=thr[:k - 1].astype(np.int64), split_gain=gain[:k - 1].copy(), leaf_value=lv[:k].copy(),
                   leaf_count=ia["leaf_count"][:k].copy(), data_leaf_index=dli)
        for key in ("split_feature_inner", "default_left", "left_child", "right_child", "internal_count"):
            out[key] = ia[key][:k - 1].copy()
        # categorical nodes: flags and the sets of bins going left (threshold_in_bin of such a node = its index among them, as in the reference's Tree)
        nic = np.zeros(max(k - 1, 1), dtype=np.int32); ncb = np.zeros((max(k - 1, 1), 8), dtype=np.uint32)
        if k > 1:
            _shim_call(_lib().gpb_hip_hist_last_tree_cat_nodes(self.h, C.c_int(k - 1), _p(nic, C.c_int), _p(ncb, C.c_uint32)))
        out["node_is_cat"] = nic[:k - 1].copy(); out["node_cat_bits"] = ncb[:k - 1].copy()
        return out

    # ---- tree scoring: leaf of a binned row, score += leaf value (out-of-bag rows, a validation matrix, new data) ----
    @staticmethod
    def node_go_left_mask(max_bin, default_bin, most_freq_bin, missing_type, default_left, threshold, cat_bits=None):
        """-> 8 words: bit b = does STORED bin b of the column go left at this node (the rule of split_leaf; cat_bits: a categorical node's set).
        max_bin = stored bins of the column - 1.  Host only: needs no handle and no device."""
        w = None if cat_bits is None else np.ascontiguousarray(cat_bits, dtype=np.uint32)
        if w is not None and w.size != 8:
            raise ValueError("cat_bits must have 8 words")
        out = np.zeros(8, dtype=np.uint32)
        _shim_call(_lib().gpb_hip_hist_node_go_left_mask(C.c_int(int(max_bin)), C.c_int(int(default_bin)), C.c_int(int(most_freq_bin)), C.c_int(int(missing_type)),
                                                         C.c_int(int(bool(default_left))), C.c_uint(int(threshold)), _p(w, C.c_uint32), _p(out, C.c_uint32)))
        return out

    def add_tree(self, tree, shrinkage=1.0):
        """Stores a tree given as what grow_tree returns (or the same arrays of a reference tree) -> its id.  Leaf values are stored as
        leaf_value * shrinkage."""
        k = int(tree["num_leaves"])
        ia = {key: np.ascontiguousarray(np.asarray(tree[key])[:max(k - 1, 0)], dtype=np.int32) for key in ("split_feature_inner", "default_left", "left_child", "right_child")}
        thr = np.ascontiguousarray(np.asarray(tree["threshold_in_bin"])[:max(k - 1, 0)], dtype=np.uint32)
        lv = np.ascontiguousarray(np.asarray(tree["leaf_value"])[:k], dtype=np.float64)
        nic = ncb = None
        if tree.get("node_is_cat") is not None:
            nic = np.ascontiguousarray(np.asarray(tree["node_is_cat"])[:max(k - 1, 0)], dtype=np.int32)
        if tree.get("node_cat_bits") is not None:
            ncb = np.ascontiguousarray(np.asarray(tree["node_cat_bits"]).reshape(-1, 8)[:max(k - 1, 0)], dtype=np.uint32)
        tid = C.c_int(-1)
        _shim_call(_lib().gpb_hip_hist_forest_add_tree(self.h, C.c_int(k), _p(ia["split_feature_inner"], C.c_int), _p(thr, C.c_uint32), _p(ia["default_left"], C.c_int),
                                                       _p(ia["left_child"], C.c_int), _p(ia["right_child"], C.c_int), _p(nic, C.c_int), _p(ncb, C.c_uint32), _p(lv),
                                                       C.c_double(shrinkage), C.byref(tid)))
        if k > 1 and tree.get("leaf_count") is not None:         # the cover counts the contributions need (the tree itself is stored either way)
            self.set_leaf_counts(tid.value, tree["leaf_count"])
        return tid.value

    def keep_last_tree(self, shrinkage=1.0):
        """Stores the last tree grow_tree has grown on this handle -> its id."""
        tid = C.c_int(-1)
        _shim_call(_lib().gpb_hip_hist_forest_keep_last_tree(self.h, C.c_double(shrinkage), C.byref(tid)))
        return tid.value

    def forest_size(self):
        k = C.c_int(0)
        _shim_call(_lib().gpb_hip_hist_forest_size(self.h, C.byref(k)))
        return k.value

    def forest_clear(self):
        _shim_call(_lib().gpb_hip_hist_forest_clear(self.h))

    def set_pred_bins(self, bins=None):
        """Attaches a second matrix (F, n_pred) uint8, feature-major, binned with the training data's mappers; None detaches."""
        if bins is None:
            _shim_call(_lib().gpb_hip_hist_set_pred_bins(self.h, C.c_int(0), None))
            self.n_pred = 0
            return
        b = np.ascontiguousarray(bins, dtype=np.uint8)
        if b.ndim != 2 or b.shape[0] != self.F:
            raise ValueError("bins must be (F, n_pred)")
        _shim_call(_lib().gpb_hip_hist_set_pred_bins(self.h, C.c_int(b.shape[1]), _p(b, C.c_uint8)))
        self.n_pred = b.shape[1]

    def _score_rows(self, rows, pred):
        n = getattr(self, "n_pred", 0) if pred else self.n
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        return n, r, (n if r is None else r.size)

    def predict_leaf(self, tree_id, rows=None, pred=False):
        """-> leaf of every listed row (None: all rows) of the training matrix or, pred=True, of the attached one in the stored tree tree_id."""
        n, r, cnt = self._score_rows(rows, pred)
        out = np.empty(cnt, dtype=np.int32)
        if r is not None and cnt == 0:
            return out
        _shim_call(_lib().gpb_hip_hist_predict_leaf(self.h, C.c_int(int(bool(pred))), C.c_int(int(tree_id)), _p(r, C.c_int), C.c_int(cnt), _p(out, C.c_int)))
        return out

    def _tree_range(self, trees):
        if trees is None:
            return 0, self.forest_size()
        if isinstance(trees, (int, np.integer)):
            return int(trees), int(trees) + 1
        return int(trees[0]), int(trees[1])

    def add_score(self, score, trees=None, rows=None, pred=False):
        """score (float64, one entry per row of the matrix) += the leaf values of the stored trees `trees` (None: all; an id; (begin, end)) for the listed
        rows (None: all), in place, in tree order; every occurrence in rows adds once."""
        n, r, cnt = self._score_rows(rows, pred)
        if not (isinstance(score, np.ndarray) and score.dtype == np.float64 and score.flags.c_contiguous and score.flags.writeable):
            raise ValueError("score must be a writable contiguous float64 array (it is updated in place)")
        if score.size != n and not (pred and n == 0):
            raise ValueError("score must have one entry per row of the matrix")
        t0, t1 = self._tree_range(trees)
        if r is not None and cnt == 0:
            return score
        _shim_call(_lib().gpb_hip_hist_add_score(self.h, C.c_int(int(bool(pred))), C.c_int(t0), C.c_int(t1), _p(r, C.c_int), C.c_int(cnt), _p(score)))
        return score

    def add_score_dev(self, score_dev_ptr, trees=None, rows=None, pred=False):
        """add_score on a device array (e.g. a float64 torch tensor's data_ptr()) over all rows of the matrix, enqueued on the handle's stream: nothing is copied and
        nothing waited for; sync() waits for the stream."""
        n, r, cnt = self._score_rows(rows, pred)
        t0, t1 = self._tree_range(trees)
        if r is not None and cnt == 0:
            return
        _shim_call(_lib().gpb_hip_hist_add_score_dev(self.h, C.c_int(int(bool(pred))), C.c_int(t0), C.c_int(t1), _p(r, C.c_int), C.c_int(cnt),
                                                     C.c_void_p(int(score_dev_ptr))))

    def add_score_bench(self, score_dev_ptr, trees=None, rows=None, pred=False, reps=20):
        """mean ms of one add_score_dev launch (HIP events; one warm-up launch first).  The scores end up with reps + 1 updates."""
        n, r, cnt = self._score_rows(rows, pred)
        t0, t1 = self._tree_range(trees)
        ms = C.c_double(0)
        _shim_call(_lib().gpb_hip_hist_add_score_bench(self.h, C.c_int(int(bool(pred))), C.c_int(t0), C.c_int(t1), _p(r, C.c_int), C.c_int(cnt),
                                                       C.c_void_p(int(score_dev_ptr)), C.c_int(int(reps)), C.byref(ms)))
        return ms.value

    # ---- per-feature contributions (TreeSHAP) of the stored trees ----
    @staticmethod
    def tree_shap_paths(tree, node_sets, leaf_count=None):
        """-> (first (num_leaves + 1), column, sets (E, 8) uint32, zero_fraction): per leaf the distinct columns on its path in order of first appearance, each
        with the set of stored bins that keep a row on the path and the product of count(child) / count(node).  node_sets: (nodes, 8) go-left sets
        (node_go_left_mask).  Host only: needs no handle and no device; the device path is built by the same function."""
        k = int(tree["num_leaves"])
        nn = max(k - 1, 0)
        ia = [np.ascontiguousarray(np.asarray(tree[key])[:nn], dtype=np.int32) for key in ("split_feature_inner", "left_child", "right_child")]
        ns = np.ascontiguousarray(np.asarray(node_sets, dtype=np.uint32).reshape(-1, 8)[:nn])
        lc = tree.get("leaf_count") if leaf_count is None else leaf_count
        lc = None if lc is None else np.ascontiguousarray(np.asarray(lc)[:k], dtype=np.int32)
        cap = 32 * k
        first = np.zeros(k + 1, dtype=np.int32); col = np.zeros(cap, dtype=np.int32); sets = np.zeros((cap, 8), dtype=np.uint32); zero = np.zeros(cap)
        _shim_call(_lib().gpb_hip_tree_shap_paths(C.c_int(k), _p(ia[0], C.c_int), _p(ia[1], C.c_int), _p(ia[2], C.c_int), _p(ns, C.c_uint32), _p(lc, C.c_int),
                                                  C.c_int(cap), _p(first, C.c_int), _p(col, C.c_int), _p(sets, C.c_uint32), _p(zero)))
        e = int(first[-1])
        return first, col[:e].copy(), sets[:e].copy(), zero[:e].copy()

    def set_leaf_counts(self, tree_id, leaf_count):
        """The cover counts of a stored tree, one per leaf (the reference's leaf_count; a node's count is the sum below it): TreeSHAP weights the branches a
        row does not take by them.  keep_last_tree records the grown tree's own counts, add_tree a dict's 'leaf_count'."""
        lc = np.ascontiguousarray(leaf_count, dtype=np.int32)
        _shim_call(_lib().gpb_hip_hist_forest_set_leaf_counts(self.h, C.c_int(int(tree_id)), _p(lc, C.c_int)))

    def tree_expected_value(self, tree_id):
        """sum over the leaves of (count / total) * stored leaf value, in leaf order (Tree::ExpectedValue); a tree of one leaf: its value."""
        v = C.c_double(0)
        _shim_call(_lib().gpb_hip_hist_tree_expected_value(self.h, C.c_int(int(tree_id)), C.byref(v)))
        return v.value

    def add_contrib(self, out, trees=None, rows=None, pred=False):
        """out (float64, (rows of the matrix, F + 1)) += the per-feature contributions of the stored trees `trees` (None: all; an id; (begin, end)) for the
        listed rows (None: all; any order, no row twice), in place: column f < F gets phi_f, column F the trees' expected values.  A row's entries receive
        their additions in (tree, leaf, path element) order onto the running value."""
        n, r, cnt = self._score_rows(rows, pred)
        if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable):
            raise GPBoostError("add_contrib: out must be a writable contiguous float64 array (it is updated in place)")
        if out.shape != (n, self.F + 1) and not (pred and n == 0):
            raise GPBoostError("add_contrib: out must have the shape (rows of the matrix, F + 1) = (%d, %d)" % (n, self.F + 1))
        t0, t1 = self._tree_range(trees)
        if r is not None and cnt == 0:
            return out
        _shim_call(_lib().gpb_hip_hist_add_contrib(self.h, C.c_int(int(bool(pred))), C.c_int(t0), C.c_int(t1), _p(r, C.c_int), C.c_int(cnt), _p(out)))
        return out

    def add_contrib_dev(self, out_dev_ptr, trees=None, rows=None, pred=False):
        """add_contrib on a device matrix (rows of the matrix x (F + 1) doubles, row-major), enqueued on the handle's stream: nothing is copied and nothing
        waited for; sync() waits for the stream."""
        n, r, cnt = self._score_rows(rows, pred)
        t0, t1 = self._tree_range(trees)
        if r is not None and cnt == 0:
            return
        _shim_call(_lib().gpb_hip_hist_add_contrib_dev(self.h, C.c_int(int(bool(pred))), C.c_int(t0), C.c_int(t1), _p(r, C.c_int), C.c_int(cnt),
                                                       C.c_void_p(int(out_dev_ptr))))

    def add_contrib_bench(self, out_dev_ptr, trees=None, rows=None, pred=False, reps=20):
        """mean ms of one add_contrib_dev launch (HIP events; one warm-up launch first).  The matrix ends up with reps + 1 updates."""
        n, r, cnt = self._score_rows(rows, pred)
        t0, t1 = self._tree_range(trees)
        ms = C.c_double(0)
        _shim_call(_lib().gpb_hip_hist_add_contrib_bench(self.h, C.c_int(int(bool(pred))), C.c_int(t0), C.c_int(t1), _p(r, C.c_int), C.c_int(cnt),
                                                         C.c_void_p(int(out_dev_ptr)), C.c_int(int(reps)), C.byref(ms)))
        return ms.value

    def pred_contrib(self, trees=None, rows=None, pred=False):
        """-> a fresh (cnt, F + 1) array in list order: the contributions of the stored trees to the listed rows (None: all) -- the shape of the reference's
        predict(..., pred_contrib=True) for one class."""
        n, r, cnt = self._score_rows(rows, pred)
        out = np.zeros((n, self.F + 1))
        self.add_contrib(out, trees=trees, rows=r, pred=pred)
        return out if r is None else out[r].copy()

    def sync(self):
        _shim_call(_lib().gpb_hip_hist_sync(self.h))

    def get_slot(self, slot):
        out = np.empty((self.total_bins, 2))
        _shim_call(_lib().gpb_hip_hist_get_slot(self.h, C.c_int(int(slot)), _p(out)))
        return out

    def build(self, data_indices=None, const_hess=1.0):
        """-> (hist[total_bins, 2] = {grad sum, hess sum}, cnt[total_bins] uint64)"""
        di = None if data_indices is None else np.ascontiguousarray(data_indices, dtype=np.int32)
        nd = self.n if di is None else di.size
        hist = np.empty((self.total_bins, 2)); cnt = np.empty(self.total_bins, dtype=np.uint64)
        _shim_call(_lib().gpb_hip_hist_build(self.h, _p(di, C.c_int32), C.c_int(nd), C.c_double(const_hess), _p(hist),
                                             _p(cnt, C.c_uint64)))
        return hist, cnt
