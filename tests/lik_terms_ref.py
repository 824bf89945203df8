"""The likelihood kernels of the Vecchia-Laplace path (gpboost_amd/csrc/laplace_kernels.hip: lik_newton_setup_kernel, lik_objective_kernel, lik_third_kernel,
lik_grad_F_kernel, lik_grad_F_map_kernel, lik_aux_grad_kernel and the device functions under them) restated per datum, once, generically over a number type.
numpy and mpmath only; nothing here touches the device.

Two number types run the same formula text (operation order of the kernels; the approximations are the reference's own: its normalLogCDF series, its digamma /
trigamma / tetragamma recurrences with their literal constants, include/GPBoost/DF_utils.h:37-98 and src/GPBoost/DF_utils.cpp:82-201, read against the kernels):
  F64  Python floats and the `math` module (the host's libm).  Records every branch decision and loop count, every argument a library function is called with,
       and whether every intermediate is finite.
  Trk  a 60-digit mpmath value plus a first-order running error bound in two parts, in units of u = 2^-53:
         E_arith  grows by |result| at every arithmetic operation (an fma counts as its two operations, which only loosens the bound), plus the input errors
                  times the partial derivatives;
         E_lib,f  one part per library function f (exp, log, log1p, erfc, lgamma, sqrt): grows by |result| at every result of f, propagated like E_arith.
       |result| is floored at 2^-1022, so a subnormal (or underflowed) result keeps the absolute error 2^-1075 of its format.
       Branches and loop counts are REPLAYED from the F64 run; where the 60-digit value (rounded to fp64, so that `erfc(..) > 0` means what it means on the
       device) would decide differently, the grid point is a defect of the grid and is recorded (the CPU test asserts there is none).
Truth is the reference's FORMULA in 60 digits, not the ideal function: at z = -37 the probit information r (z + r) is only good to 1e-10 as a formula, and the
bound follows that through the propagated terms.

Bound of one output:  u (E_arith + sum_f eps_f E_lib,f),  eps_f = relative error of library function f in units of u (1 for a correctly rounded result).
Row sums over re_ptr and the weights are tracked additions (the running error bound of the kernel's own chain).  The two workgroup reductions add Higham's
gamma(k) sum |terms| (Accuracy and Stability of Numerical Algorithms, Lemma 3.1 + section 4.2), k counted from the kernel:
  lik_objective_kernel  a lane's chain `ll += wt * loglik` over the data of its rows i = lane, lane + 1024, ..: k_chain = the largest number of data of one lane;
                        then block_reduce2: ten levels (512 .. 1), one addition each.                        k = k_chain + 10
                        q = fma(Bx (1 / D), Bx, q): the reciprocal and the product are tracked in the term; chain = rows of a lane.   k = ceil(n / 1024) + 10
  lik_aux_grad_kernel   `e += ..` / `dsum = fma(.., diag, dsum)` / `isum = fma(.., svi, isum)`: one rounding per datum of the lane, then the tree.     k = k_chain + 10
The per-row objective (lap_objective on one row, n = 1): lane 0 holds the chain, every other lane adds exact zeros.

The grid (LOCATIONS, RESPONSES, AUX, allowed()) is explicit; a point is in a likelihood's grid only if every fp64 intermediate of the restatement is finite, which
the CPU test asserts for everything allowed() admits.  Probit arguments in [-38.6, -37.5] are left out (erfc is subnormal there: the reference's own value has a
few bits); the series branch is entered from |z| = 40 down the left tail.

Measured (worst |error| / bound per likelihood and output; CPU = the F64 restatement at eps_f = 1, GPU = MI355X at the probe's eps_f):
RATIO_TABLE_BEGIN
eps_f measured on the MI355X over the arguments the grid hands each function (worst relative error in u; eps_f = max(2, 2 x worst)):
  eps_exp    = 2.000   (53 arguments in [-4.5e+04, 300], worst 0.932 u at -0.4)
  eps_log    = 2.000   (377 arguments in [3.91e-306, 1.14e+26], worst 0.964 u at 3056.5)
  eps_log1p  = 2.000   (28 arguments in [-1, 1], worst 0.669 u at -1e-09)
  eps_erfc   = 3.524   (14 arguments in [-0, 212], worst 1.762 u at 8.48528)
  eps_lgamma = 3.404   (107 arguments in [1e-15, 1e+04], worst 1.702 u at 9525.74)
  eps_sqrt   = 2.000   (377 arguments in [3.91e-306, 1.14e+26], worst 1.000 u at 1)
  (no kernel of this family calls sqrt; it is probed at the arguments of log)
likelihood         run       W    rhs     dw    rdw    dW3 ll_row  gradF out2_0 out2_1 out3_0 out3_1 out3_2
bernoulli_logit    CPU    0.58   0.60   0.94   0.57   0.46   0.38   0.52   0.05   0.13      -      -      -
bernoulli_logit    GPU    0.57   0.59   0.94   0.57   0.46   0.38   0.52   0.05   0.13      -      -      -
bernoulli_probit   CPU    0.32   0.32   0.66   0.47   0.29   0.60   0.32   0.06   0.06      -      -      -
bernoulli_probit   GPU    0.29   0.29   0.66   0.47   0.29   0.60   0.31   0.06   0.06      -      -      -
poisson            CPU    0.58   0.72   0.58   0.57   0.58   0.51   0.57   0.06   0.05      -      -      -
poisson            GPU    0.41   0.72   0.57   0.57   0.41   0.24   0.57   0.06   0.05      -      -      -
gamma              CPU    0.53   0.53   0.64   0.55   0.42   0.38   0.47   0.08   0.11   0.08   0.10   0.05
gamma              GPU    0.45   0.53   0.64   0.55   0.46   0.38   0.47   0.07   0.11   0.08   0.10   0.04
negative_binomial  CPU    0.36   0.53   0.76   0.58   0.38   0.52   0.62   0.06   0.15   0.12   0.02   0.06
negative_binomial  GPU    0.34   0.53   0.76   0.58   0.35   0.41   0.62   0.06   0.15   0.12   0.02   0.11
beta               CPU    0.38   0.39   0.71   0.53   0.22   0.45   0.46   0.35   0.13   0.02   0.00   0.03
beta               GPU    0.38   0.39   0.71   0.53   0.22   0.45   0.44   0.35   0.13   0.02   0.01   0.02
t                  CPU    0.15   0.28   0.82   0.58   0.00   1.00   0.54   0.75   0.11   0.07   0.75   0.00
t                  GPU    0.15   0.25   0.82   0.58   0.00   1.00   0.54   0.75   0.11   0.07   0.75   0.00
lognormal          CPU    0.37   0.49   0.91   0.55   0.00   0.42   0.48   0.08   0.08   0.06   0.00   0.00
lognormal          GPU    0.37   0.39   0.91   0.55   0.00   0.39   0.42   0.06   0.08   0.06   0.00   0.00
gaussian_latent    CPU    0.37   0.37   0.80   0.63   0.00   0.33   0.51   0.08   0.11   0.10   0.00   0.00
gaussian_latent    GPU    0.37   0.38   0.80   0.63   0.00   0.33   0.51   0.08   0.11   0.10   0.00   0.00
(t, ll_row 1.00: 0.998, log(1 + 3.4e-16) at y - x = 1e-3, scale 1e4 -- the rounding of 1 + x is the whole value, and the bound says so)
RATIO_TABLE_END
"""
import math
import operator

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 60
U = 2.0 ** -53
TINY = 2.0 ** -1022
LIB = ("exp", "log", "log1p", "erfc", "lgamma", "sqrt")
_MPFN = {"exp": MP.exp, "log": MP.log, "log1p": MP.log1p, "erfc": MP.erfc, "lgamma": MP.loggamma, "sqrt": MP.sqrt}
_CMP = {"lt": operator.lt, "le": operator.le, "gt": operator.gt, "ge": operator.ge, "eq": operator.eq}
_HALF_DENORM = MP.mpf(2) ** -1075
(LOGIT, PROBIT, POISSON, GAMMA, NEGBIN, BETA, TLIK, LOGNORMAL, GAUSS) = range(9)
LIK_NAMES = ("bernoulli_logit", "bernoulli_probit", "poisson", "gamma", "negative_binomial", "beta", "t", "lognormal", "gaussian_latent")
HAS_AUX = (False, False, False, True, True, True, True, True, True)
INT_RESP = (True, True, True, False, True, False, False, False, False)       # set_labels / counts accepted
REAL_RESP = (True, True, False, True, False, True, True, True, True)        # a real response accepted (lik_table.h: lik_accepts_real)


def gamma(k):
    return k * U / (1.0 - k * U)


def to_f64(v):
    """a 60-digit value as the fp64 format would hold it (what a comparison on the device sees)"""
    if abs(v) < _HALF_DENORM:
        return 0.0
    try:
        return float(v)
    except OverflowError:
        return math.copysign(math.inf, float(MP.sign(v)))


# thresholds of digamma_dev / trigamma_dev / tetragamma_dev (small-argument branches, ends of the recurrences) -> the smallest relative distance of a compared value
THRESHOLD_DIST = {0.000001: math.inf, 0.0001: math.inf, 5.0: math.inf, 8.0: math.inf, 8.5: math.inf}


# ---- the fp64 type -------------------------------------------------------------------------------------------------------------------------------
class F64(object):
    __slots__ = ("v", "c")

    def __init__(self, v, c):
        self.v, self.c = v, c
        if not math.isfinite(v):
            c.finite = False

    def __float__(self):
        return self.v

    def _o(self, o):
        return o.v if isinstance(o, F64) else float(o)

    def __neg__(self):
        return F64(-self.v, self.c)

    def __add__(self, o):
        return F64(self.v + self._o(o), self.c)
    __radd__ = __add__

    def __sub__(self, o):
        return F64(self.v - self._o(o), self.c)

    def __rsub__(self, o):
        return F64(self._o(o) - self.v, self.c)

    def __mul__(self, o):
        return F64(self.v * self._o(o), self.c)
    __rmul__ = __mul__

    @staticmethod
    def _div(a, b):
        try:
            return a / b
        except ZeroDivisionError:
            return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)

    def __truediv__(self, o):
        return F64(self._div(self.v, self._o(o)), self.c)

    def __rtruediv__(self, o):
        return F64(self._div(self._o(o), self.v), self.c)


class Ctx64(object):
    kind = "f64"

    def __init__(self, mut=None, args=None):
        self.trace, self.finite, self.mut, self.args = [], True, mut, args

    def num(self, v):
        return v if isinstance(v, F64) else F64(float(v), self)

    def branch(self, op, a, b):
        fa, fb = float(a), float(b)
        r = _CMP[op](fa, fb)
        self.trace.append(r)
        if fb in THRESHOLD_DIST and self.mut is None:       # how close an argument of the gamma family comes to one of its thresholds
            THRESHOLD_DIST[fb] = min(THRESHOLD_DIST[fb], abs(fa - fb) / fb)
        return r

    def lib(self, name, a):
        a = float(a)
        if self.args is not None:
            self.args[name].add(a)
        try:
            r = getattr(math, name)(a)
        except (OverflowError, ValueError):
            r = math.nan
        return F64(r, self)


# ---- the tracked type ----------------------------------------------------------------------------------------------------------------------------
def _merge(e1, s1, e2, s2):
    if not e1 and not e2:
        return e1
    out = {k: s1 * v for k, v in e1.items()}
    for k, v in e2.items():
        out[k] = out.get(k, 0.0) + s2 * v
    return out


_NOLIB = {}


class Trk(object):
    __slots__ = ("v", "f", "ea", "el", "c")

    def __init__(self, v, f, ea, el, c):
        self.v, self.f, self.ea, self.el, self.c = v, f, ea, el, c

    def __float__(self):
        return self.f

    def _o(self, o):
        return o if isinstance(o, Trk) else Trk(MP.mpf(float(o)), float(o), 0.0, _NOLIB, self.c)

    def __neg__(self):
        return Trk(-self.v, -self.f, self.ea, self.el, self.c)

    def _add(self, b, sign):
        v = self.v + b.v if sign > 0 else self.v - b.v
        f = to_f64(v)
        return Trk(v, f, self.ea + b.ea + max(abs(f), TINY), _merge(self.el, 1.0, b.el, 1.0), self.c)

    def __add__(self, o):
        return self._add(self._o(o), 1)
    __radd__ = __add__

    def __sub__(self, o):
        return self._add(self._o(o), -1)

    def __rsub__(self, o):
        return self._o(o)._add(self, -1)

    def __mul__(self, o):
        b = self._o(o)
        v = self.v * b.v
        f = to_f64(v)
        sa, sb = abs(b.f), abs(self.f)
        return Trk(v, f, sa * self.ea + sb * b.ea + max(abs(f), TINY), _merge(self.el, sa, b.el, sb), self.c)
    __rmul__ = __mul__

    @staticmethod
    def _quot(a, b):
        v = a.v / b.v
        f = to_f64(v)
        # first order: |f| (rel(a) + rel(b)); formed from the relative errors so that neither a huge 1 / |b|^2 overflows nor a tiny quotient is lost
        af, ib = abs(f), (1.0 / abs(b.f) if b.f != 0.0 else math.inf)
        if a.f != 0.0 and f != 0.0:
            ra, ma = 1.0 / abs(a.f), af
        else:
            ra, ma = ib, 1.0
        ea = (ma * (a.ea * ra) if a.ea else 0.0) + (af * (b.ea * ib) if b.ea else 0.0) + max(af, TINY)
        el = {k: ma * (e * ra) for k, e in a.el.items()}
        for k, e in b.el.items():
            el[k] = el.get(k, 0.0) + af * (e * ib)
        return Trk(v, f, ea, el, a.c)

    def __truediv__(self, o):
        return Trk._quot(self, self._o(o))

    def __rtruediv__(self, o):
        return Trk._quot(self._o(o), self)


class CtxT(object):
    kind = "trk"
    mut = None

    def __init__(self, trace):
        self.trace, self.pos, self.defects = trace, 0, []

    def num(self, v):
        return v if isinstance(v, Trk) else Trk(MP.mpf(float(v)), float(v), 0.0, _NOLIB, self)

    def branch(self, op, a, b):
        want = self.trace[self.pos]
        self.pos += 1
        fa = a.f if isinstance(a, Trk) else float(a)
        fb = b.f if isinstance(b, Trk) else float(b)
        if _CMP[op](fa, fb) != want:
            self.defects.append((op, fa, fb))
        return want

    def lib(self, name, a):
        a = self.num(a)
        v = _MPFN[name](a.v)
        f = to_f64(v)
        ea, el = 0.0, {}
        if a.ea or a.el:       # the argument's own error times |f'|
            if name == "exp":
                d = abs(f)
            elif name == "log":
                d = 1.0 / abs(a.f)
            elif name == "log1p":
                d = 1.0 / abs(1.0 + a.f)
            elif name == "erfc":
                d = to_f64(2 / MP.sqrt(MP.pi) * MP.exp(-a.v * a.v))
            elif name == "lgamma":
                d = abs(to_f64(MP.digamma(a.v)))
            else:
                d = 0.5 / abs(f)
            ea = d * a.ea
            el = {k: d * e for k, e in a.el.items()}
        el[name] = el.get(name, 0.0) + max(abs(f), TINY)
        return Trk(v, f, ea, el, self)


# ---- the formulas, written once (M: Ctx64 or CtxT) -----------------------------------------------------------------------------------------------------
def sigmoid_stable(M, x):
    if M.branch("ge", x, 0.0):
        t = M.lib("exp", -x)
        return 1.0 / (1.0 + t)
    t = M.lib("exp", x)
    return t / (1.0 + t)


def softplus(M, x):
    if M.mut == "naive_softplus":
        return M.lib("log", 1.0 + M.lib("exp", x))
    a = x if M.branch("ge", x, 0.0) else -x                 # fabs, fmax: exact
    pos = x if M.branch("gt", x, 0.0) else M.num(0.0)
    return M.lib("log1p", M.lib("exp", -a)) + pos


def normal_log_cdf(M, x):
    if M.branch("lt", x, 0.0):
        e = M.lib("erfc", -x * 0.70710678118654752440)
        if M.branch("gt", e, 0.0):
            return M.lib("log", 0.5) + M.lib("log", e)
        u = -x
        u2 = u * u
        series = 1.0 - 1.0 / u2 if M.mut == "series_no_u4" else 1.0 - 1.0 / u2 + 3.0 / (u2 * u2)
        return -0.5 * u2 - M.lib("log", u) - 0.5 * M.lib("log", 2 * 3.14159265358979323846) + M.lib("log", series)
    Q = 0.5 * M.lib("erfc", x * 0.70710678118654752440)
    if M.branch("eq", Q, 0.0):
        return M.num(0.0)
    return M.lib("log", 1.0 - Q) if M.mut == "log_for_log1p" else M.lib("log1p", -Q)


def inv_mills_phi(M, z):
    return M.lib("exp", (-z * z / 2. - 0.91893853320467274178) - normal_log_cdf(M, z))


def digamma(M, x):
    if M.branch("le", x, 0.000001):
        return -0.57721566490153286060 - 1.0 / x + 1.6449340668482264365 * x
    v = M.num(0.0)
    while M.branch("lt", x, 8.5):
        v = v - 1.0 / x
        x = x + 1.0
    r = 1.0 / x
    v = v + (M.lib("log", x) - 0.5 * r)
    r = r * r
    c12, c120, c252, c240, c132 = (M.num(1.0) / k for k in (12.0, 120.0, 252.0, 240.0, 132.0))
    return v - r * (c12 - r * (c120 - r * (c252 - r * (c240 - r * c132))))


def trigamma(M, x):
    if M.branch("le", x, 0.0001):
        return 1.0 / x / x
    value, z = M.num(0.0), x
    while M.branch("lt", z, 5.0):
        value = value + 1.0 / z / z
        z = z + 1.0
    y = 1.0 / z / z
    b2 = 0.1666656667 if M.mut == "trigamma_const" else 0.1666666667
    return value + 0.5 * y + (1.0 + y * (b2 + y * (-0.03333333333 + y * (0.02380952381 + y * -0.03333333333)))) / z


def tetragamma(M, x):
    if M.branch("le", x, 1e-4):
        return -2.0 / (x * x * x)
    z, value = x, M.num(0.0)
    while M.branch("lt", z, 8.0):
        value = value - 2.0 / (z * z * z)
        z = z + 1.0
    z2 = z * z
    z3 = z2 * z
    z4 = z2 * z2
    z6 = z4 * z2
    z8 = z4 * z4
    z10 = z8 * z2
    s3 = 1.0 if M.mut == "tetragamma_sign" else -1.0
    return value + (-1.0 / z2 + s3 / z3 - 0.5 / z4 + 1.0 / (6.0 * z6) - 1.0 / (6.0 * z8) + 3.0 / (10.0 * z10))


def sigmoid_clamped(M, x):
    lo = 1e-10 if M.mut == "clamp_1e10" else 1e-12
    mu = sigmoid_stable(M, x)
    if M.branch("lt", mu, lo):
        mu = M.num(lo)
    if M.branch("gt", mu, 1.0 - lo):
        mu = M.num(1.0 - lo)
    return mu


def datum_core(M, lik, y, x, aux, aux2):
    """Everything the kernels compute from ONE datum before a weight touches it: ll (lik_loglik), g, w (lik_grad_info), t3 (lik_third) and the pieces of the
    lik_aux_grad_kernel summands.  y, x, aux, aux2: numbers of M.  (The kernels evaluate shared sub-expressions once per kernel; the same inputs give the same bits.)"""
    L, one = M.lib, 1.0
    c = {}
    if lik == LOGIT:
        p = sigmoid_stable(M, x)
        c["ll"] = y * x - softplus(M, x)
        c["g"] = y - p
        c["w"] = p * (one - p)
        c["t3"] = -p * (one - p) * (2.0 * p - one)
    elif lik == PROBIT:
        y0, y1 = M.branch("eq", y, 0.0), M.branch("eq", y, 1.0)
        x2 = x * x
        if y0 or y1:
            label1 = y1 if M.mut != "probit_swap" else y0
            z = x if label1 else -x
            r = inv_mills_phi(M, z)
            c["ll"] = normal_log_cdf(M, z)
            c["g"] = r if label1 else -r
            c["w"] = r * (z + r)
            if y0:
                q = inv_mills_phi(M, -x)
                c["t3"] = -q * (one - x2 + q * (3.0 * x - 2.0 * q))
            else:
                rr = inv_mills_phi(M, x)
                c["t3"] = -rr * (x2 - one + rr * (3.0 * x + 2.0 * rr))
        else:
            c["ll"] = y * normal_log_cdf(M, x) + (one - y) * normal_log_cdf(M, -x)
            r1, r0 = inv_mills_phi(M, x), inv_mills_phi(M, -x)
            c["g"] = y * r1 + (one - y) * -r0
            c["w"] = y * r1 * (x + r1) + (one - y) * -r0 * (x - r0)
            c["t3"] = y * (-r1 * (x2 - one + r1 * (3.0 * x + 2.0 * r1))) + (one - y) * (-r0 * (one - x2 + r0 * (3.0 * x - 2.0 * r0)))
    elif lik == POISSON:
        e = L("exp", x)
        c["ll"] = y * x - e
        c["g"] = y - e
        c["w"] = e
        c["t3"] = e
    elif lik == GAMMA:
        q = y * L("exp", -x)
        c["ll"] = -aux * (x + q)
        c["g"] = aux * (q - one)
        c["w"] = aux * q
        c["t3"] = -aux * y * L("exp", -x)
        c["q"] = q
    elif lik == NEGBIN:
        mu = L("exp", x)
        mr = mu + aux
        c["ll"] = y * x - (y + aux) * L("log", mu + aux)
        c["g"] = y - (y + aux) / mr * mu
        c["w"] = (y + aux) * mu * aux / (mr * mr)
        dm = aux - mu if M.mut == "negbin_aux_minus_mu" else mu - aux
        c["t3"] = -(y + aux) * mu * aux * dm / (mr * mr * mr)
        r, yr = aux, y + aux
        c["e"] = r * (-digamma(M, yr) + L("log", mr) + yr / mr)
        q = mu * r / (mr * mr)
        c["d"] = -q * (y * (r - mu) - 2.0 * r * mu) / mr
        c["i"] = q * (y - mu)
    elif lik == BETA:
        mu = sigmoid_clamped(M, x)
        om = one - mu
        logy = L("log", y)
        l1py = L("log1p", -y)
        logit_y = logy - l1py
        a1, a2 = om * aux, mu * aux
        dig1, dig2, tri1, tri2, tet1, tet2 = digamma(M, a1), digamma(M, a2), trigamma(M, a1), trigamma(M, a2), tetragamma(M, a1), tetragamma(M, a2)
        c["ll"] = -L("lgamma", a2) - L("lgamma", a1) + (a2 - one) * logy + (a1 - one) * l1py
        C = dig1 - dig2 + logit_y
        c["g"] = aux * mu * om * C
        h1 = -aux * aux * mu * mu * om * om * (tri1 + tri2)
        h2 = aux * mu * om * (one - 2.0 * mu) * C
        c["w"] = -(h1 + h2)
        d = mu * om
        S, Dlt = tri1 + tri2, tet2 - tet1
        term_trigam = 3.0 * aux * aux * d * d * (one - 2.0 * mu) * S
        term_tetragam = aux * aux * aux * d * d * d * Dlt
        gp = d * ((one - 2.0 * mu) * (one - 2.0 * mu) - 2.0 * d)
        c["t3"] = term_trigam + term_tetragam + -aux * gp * C
        r = aux
        c["e"] = digamma(M, r) - mu * dig2 - om * dig1 + mu * logy + om * l1py
        Dlt_tri, Dlt_tet = om * tri1 - mu * tri2, om * tet1 + mu * tet2
        c["i"] = -(r * d * C + r * r * d * Dlt_tri)
        term1, term2 = 2.0 * r * r * d * d * S, r * r * r * d * d * Dlt_tet
        term3, term4 = -r * d * (one - 2.0 * mu) * C, -r * r * d * (one - 2.0 * mu) * Dlt_tri
        c["d"] = term1 + term2 + term3 + term4
    elif lik == TLIK:
        res = y - x
        c["ll"] = -(aux2 + one) / 2.0 * L("log", one + (y - x) * (y - x) / (aux2 * aux * aux))
        c["g"] = (aux2 + one) * res / (aux2 * aux * aux + res * res)
        c["w"] = (aux2 + one) / (aux2 + 3.0) / (aux * aux)
        c["t3"] = M.num(0.0)
        nu = aux2
        nu_sigma2, res_sq = nu * aux * aux, (y - x) * (y - x)
        c["e_num"], c["e_den"] = nu + one, nu_sigma2 / res_sq + one
        c["d"] = -nu * L("log", one + res_sq / nu_sigma2) + (nu + one) / (one + nu_sigma2 / res_sq)
    elif lik == LOGNORMAL:
        z = L("log", y) - (x - 0.5 * aux)
        c["ll"] = -0.5 * z * z / aux
        c["g"] = (L("log", y) - (x - 0.5 * aux)) / aux
        c["w"] = one / aux
        c["t3"] = M.num(0.0)
        c["e"] = (z + one) * 0.5 - (z * z) / (2.0 * aux)
    else:
        res = y - x
        c["ll"] = -res * res / 2.0 / aux
        c["g"] = (y - x) / aux
        c["w"] = one / aux
        c["t3"] = M.num(0.0)
        c["res"] = res
    return c


def row_terms(M, lik, cores, wts, xs, mode, D, dld, sv, Bx, aux, has_ptr):
    """One row of every kernel from its data's cores (datum_core), in the kernels' order.  wts: the data's weights or None; xs: the data's locations.
    -> dict: W, rhs, dw, rdw, dW3, ll_row, q_term, gradF (list), and the per-datum terms of the reductions: ll_t, e_t, d_t, i_t (lists)"""
    one = M.num(1.0)
    wt = (lambda d: wts[d]) if wts is not None else (lambda d: one)
    o = {}
    if has_ptr:
        gr, w = M.num(0.0), M.num(0.0)
        for d, c in enumerate(cores):
            gr = gr + wt(d) * c["g"]
            w = w + wt(d) * c["w"]
    else:
        gr, w = cores[0]["g"], cores[0]["w"]
        if wts is not None:
            gr, w = gr * wts[0], w * wts[0]
    o["W"] = w
    o["rhs"] = w * mode + gr
    o["dw"] = 1.0 / D + w
    o["rdw"] = 1.0 / o["dw"]
    o["ll_t"] = [c["ll"] if M.mut == "dropped_weight" else wt(d) * c["ll"] for d, c in enumerate(cores)]
    ll = M.num(0.0)
    for t in o["ll_t"]:
        ll = ll + t
    o["ll_row"] = ll
    if Bx is not None:
        o["q_term"] = Bx * (1.0 / D) * Bx
    if has_ptr:
        t3 = M.num(0.0)
        for d, c in enumerate(cores):
            t3 = t3 + wt(d) * c["t3"]
    else:
        t3 = wt(0) * cores[0]["t3"]
    o["dW3"] = t3
    diag = None
    if has_ptr or HAS_AUX[lik]:
        if M.mut == "no_t3_guard":
            diag = dld / t3
        else:
            diag = M.num(0.0) if M.branch("eq", t3, 0.0) else dld / t3
    if has_ptr:
        o["gradF"] = [-(wt(d) * c["g"]) + 0.5 * (wt(d) * c["t3"]) * diag - (wt(d) * c["w"]) * sv for d, c in enumerate(cores)]
    else:
        o["gradF"] = [-gr + 0.5 * dld - w * sv]
    if HAS_AUX[lik]:
        e_t, d_t, i_t = [], [], []
        for d, c in enumerate(cores):
            wd = wt(d)
            if lik == LOGNORMAL:
                e_t.append(wd * c["e"])
            elif lik == GAUSS:
                e_t.append(wd * c["res"] * c["res"])
            elif lik == TLIK:
                e_t.append(-(wd * c["e_num"] / c["e_den"]))
                d_t.append(wd * c["d"])
            elif lik == GAMMA:
                e_t.append(wd * (xs[d] + c["q"]))
                s2 = (one if M.mut == "gamma_single_weight" else wd) * (aux * (c["q"] - 1.0))
                d_t.append(wd * (s2 + aux) * diag)
                i_t.append(s2 * sv)
            else:       # beta, negative binomial
                e_t.append(wd * c["e"])
                d_t.append(wd * c["d"] * diag)
                i_t.append(wd * c["i"] * sv)
        o["e_t"], o["d_t"], o["i_t"] = e_t, d_t, i_t
    return o


# ---- the grid ------------------------------------------------------------------------------------------------------------------------------------------
LOCATIONS = (0.0, 0.4, -0.4, 3.0, -3.0, 8.2, -8.2, 8.4, -8.4, 12.0, -12.0, 20.0, -20.0, 27.0, -27.0, 28.0, -28.0, 37.4, -37.4, 40.0, -40.0, 60.0, -60.0, 300.0, -300.0)
RESPONSES = {
    LOGIT: (0.0, 1.0, 0.3, 0.999), PROBIT: (0.0, 1.0, 0.3, 0.999), POISSON: (0.0, 1.0, 7.0, 1e4), NEGBIN: (0.0, 1.0, 7.0, 1e4),
    BETA: (1e-9, 0.01, 0.5, 0.93, 1.0 - 1e-9), GAMMA: (1e-8, 1.5, 1e6), LOGNORMAL: (1e-8, 1.5, 1e6), TLIK: (1e-3, -1e-3, 50.0, -50.0), GAUSS: (1e-3, -1e-3, 50.0, -50.0),
}
# (aux, aux2) per likelihood: four settings, one per pair of cases; the second is the t likelihood's degrees of freedom
AUX = {
    LOGIT: ((1.0, 2.0),) * 4, PROBIT: ((1.0, 2.0),) * 4, POISSON: ((1.0, 2.0),) * 4,
    GAMMA: ((1e-3, 2.0), (0.7, 2.0), (50.0, 2.0), (1e4, 2.0)), NEGBIN: ((1e-3, 2.0), (0.7, 2.0), (50.0, 2.0), (1e4, 2.0)),
    BETA: ((1e-3, 2.0), (0.7, 2.0), (50.0, 2.0), (1e4, 2.0)), TLIK: ((1e-3, 1e4), (0.7, 3.5), (50.0, 1e-3), (1e4, 30.0)),
    LOGNORMAL: ((1e-3, 2.0), (0.7, 2.0), (50.0, 2.0), (1e4, 2.0)), GAUSS: ((1e-3, 2.0), (0.7, 2.0), (50.0, 2.0), (1e4, 2.0)),
}
FIXED_EFFECTS = (0.25, -1.5, 0.0078125, 3.0, -0.625)
SHAPES = (1, 63, 257, 1500)
N_EACH_MAX = 400


def allowed(lik, loc, y, has_ptr=False):
    """The explicit exclusions of the grid.
    negative binomial: exp(300) cubed overflows in the third derivative.
    logit with re_ptr: from 37.4 up p rounds to exactly 1 and the row's third derivative to exactly 0, while the formula's is 1e-17: the `t3 == 0` guard of
    lik_grad_F_map_kernel would decide differently in 60 digits.  (Without re_ptr the same locations stay in: nothing divides by the sum there.)
    probit: arguments in [-38.6, -37.5] (no location of the grid lies there; kept as the rule for any location added later)."""
    if lik == NEGBIN:
        return loc <= 60.0
    if lik == LOGIT and has_ptr:
        return loc < 37.0
    if lik == PROBIT:
        return not 37.5 <= abs(loc) <= 38.6
    return True


def grid_points(lik, has_ptr=False):
    return [(y, loc) for loc in LOCATIONS for y in RESPONSES[lik] if allowed(lik, loc, y, has_ptr)]


def cases(lik):
    """(n, has_ptr, has_weights, has_fe, real_response, aux index): every shape with and without re_ptr, weights, fixed effects and, where the table allows both,
    with the int and the real response; every aux setting at two shapes."""
    flags = {1: (0, 0, 0), 63: (0, 1, 0), 257: (0, 0, 1), 1500: (0, 1, 1)}
    aux_of = {1: (1, 3), 63: (0, 2), 257: (0, 1), 1500: (2, 3)}
    out = []
    for n in SHAPES:
        p, w, f = flags[n]
        for k in range(2):
            has = (p ^ k, w ^ k, f ^ k)
            real = REAL_RESP[lik] and (not INT_RESP[lik] or k == (n in (63, 1500)))
            out.append((n, bool(has[0]), bool(has[1]), bool(has[2]), bool(real), aux_of[n][k]))
    return out


def _weight(j):
    return (1.0, 0.0, 2.5, 0.37, 1.0, 3.0, 0.0625)[j % 7] if j % 11 else 0.0


class Case(object):
    """The arrays of one call of the test entry, and the row templates they repeat.  Rows cycle through the templates of the grid, so that the tracked run costs one
    evaluation per template whatever n is; D, dld, sv, Bx and the weights are fixed per template."""

    def __init__(self, lik, n, has_ptr, has_w, has_fe, real, aux_idx):
        self.lik, self.n, self.has_ptr, self.has_w, self.has_fe, self.real, self.aux_idx = lik, n, has_ptr, has_w, has_fe, real, aux_idx
        self.aux, self.aux2 = AUX[lik][aux_idx]
        pts = grid_points(lik, has_ptr)
        if not real:       # the int response carries labels and counts only
            pts = [p for p in pts if float(p[0]).is_integer()]
        rng = np.random.default_rng(1000 * lik + 7)
        G = len(pts)
        self.templates = []
        j = 0
        t = 0
        while j < G:
            if has_ptr and t % 13 == 5:       # a random effect without data: an empty row
                self.templates.append(dict(ys=[], fes=[], wts=[], mode=float(pts[j][1]), D=float(10.0 ** rng.uniform(-3, 3)), dld=float(rng.standard_normal()),
                                           sv=float(rng.standard_normal()), Bx=float(rng.standard_normal())))
                t += 1
                continue
            cnt = 1 + (t % 5) if has_ptr else 1
            loc = pts[j][1]
            # the data of a row share its location: the following grid points lend their responses
            ys = [pts[(j + k) % G][0] for k in range(cnt)]
            ys = [y for y in ys if allowed(lik, loc, y, has_ptr)] or [pts[j][0]]
            fes = [FIXED_EFFECTS[t % 5]] * len(ys) if has_fe else None       # every datum of the row lands next to the row's grid location
            mode = loc - fes[0] if has_fe else loc
            self.templates.append(dict(ys=ys, fes=fes, mode=float(mode), wts=[_weight(t + 3 * k) for k in range(len(ys))] if has_w else None,
                                       D=float(10.0 ** rng.uniform(-3, 3)), dld=float(rng.standard_normal()), sv=float(rng.standard_normal()),
                                       Bx=float(rng.standard_normal())))
            j += cnt
            t += 1
        T = len(self.templates)
        self.row_t = np.arange(n) % T
        cnts = np.array([len(self.templates[k]["ys"]) for k in self.row_t])
        self.re_ptr = np.concatenate([[0], np.cumsum(cnts)]).astype(np.int32)
        self.n_data = int(self.re_ptr[-1])
        self.n_each = min(n, N_EACH_MAX)
        cat = lambda key: np.array([v for k in self.row_t for v in self.templates[k][key]], dtype=np.float64)
        per_row = lambda key: np.array([self.templates[k][key] for k in self.row_t], dtype=np.float64)
        self.y = cat("ys")
        self.weights = cat("wts") if has_w else None
        self.fe = cat("fes") if has_fe else None
        self.mode, self.D, self.dld, self.sv, self.Bx = (per_row(k) for k in ("mode", "D", "dld", "sv", "Bx"))
        # a lane's chain in the two one-workgroup reductions: the data of its rows lane, lane + 1024, ...
        lane_data = np.zeros(1024, dtype=np.int64)
        np.add.at(lane_data, np.arange(n) % 1024, cnts)
        self.k_chain = int(lane_data.max())
        self.k_rows = (n + 1023) // 1024

    def entry_kwargs(self):
        kw = dict(lik=self.lik, mode=self.mode, D=self.D, dld=self.dld, sv=self.sv, Bx=self.Bx, re_ptr=self.re_ptr if self.has_ptr else None, weights=self.weights,
                  fixed_effects=self.fe, aux=self.aux, aux2=self.aux2, n_each=self.n_each)
        kw["y_real" if self.real else "y_int"] = self.y if self.real else self.y.astype(np.int32)
        return kw


# ---- evaluation: both number types per template, cached ------------------------------------------------------------------------------------------------
LIB_ARGS = {f: set() for f in LIB}       # every argument the F64 run hands to a library function, over everything evaluated so far
_core_cache, _row_cache = {}, {}


class Val(object):
    """one output: the fp64 restatement's value, the truth as a double-double, and the two parts of the bound"""
    __slots__ = ("f64", "hi", "lo", "ea", "el")

    def __init__(self, a, t):
        self.f64 = a.v
        self.hi = to_f64(t.v)
        self.lo = to_f64(t.v - MP.mpf(self.hi)) if math.isfinite(self.hi) else 0.0
        self.ea = t.ea
        self.el = np.array([t.el.get(f, 0.0) for f in LIB])


def eval_core(lik, y, mode, fe, aux, aux2, mut=None):
    """-> (F64 core, tracked core, finite, defects) of one datum at location mode (+ fe); mut: the F64 run alone, mutated (not cached)"""
    key = (lik, y, mode, fe, aux, aux2)
    if mut is None and key in _core_cache:
        return _core_cache[key]
    M = Ctx64(mut=mut, args=LIB_ARGS if mut is None else None)
    x = M.num(mode) + fe if fe is not None else M.num(mode)
    a = datum_core(M, lik, M.num(y), x, M.num(aux), M.num(aux2))
    a["x"] = x
    if mut is not None:
        return a, None, M.finite, []
    T = CtxT(M.trace)
    xt = T.num(mode) + fe if fe is not None else T.num(mode)
    t = datum_core(T, lik, T.num(y), xt, T.num(aux), T.num(aux2)) if M.finite else None
    if t is not None:
        t["x"] = xt
        assert T.pos == len(M.trace)
    _core_cache[key] = (a, t, M.finite, T.defects)
    return _core_cache[key]


def eval_row(case, k, mut=None):
    """template k of the case -> (dict name -> Val or list of Val, finite, defects); with mut: dict name -> float or list of floats of the mutated F64 run"""
    key = (case.lik, case.has_ptr, case.has_w, case.has_fe, case.aux_idx, case.real, k)
    if mut is None and key in _row_cache:
        return _row_cache[key]
    tp = case.templates[k]
    cores = [eval_core(case.lik, y, tp["mode"], tp["fes"][d] if case.has_fe else None, case.aux, case.aux2, mut) for d, y in enumerate(tp["ys"])]
    finite = all(c[2] for c in cores)
    defects = [x for c in cores for x in c[3]]
    res = []
    trace = None
    for which in (0, 1):
        if which == 1 and (mut is not None or not finite):
            break
        M = Ctx64(mut=mut) if which == 0 else CtxT(trace)
        num = M.num
        r = row_terms(M, case.lik, [c[which] for c in cores], [num(v) for v in tp["wts"]] if case.has_w else None, [c[which]["x"] for c in cores],
                      num(tp["mode"]), num(tp["D"]), num(tp["dld"]), num(tp["sv"]), num(tp["Bx"]), num(case.aux), case.has_ptr)
        if which == 0:
            trace, finite = M.trace, finite and M.finite
        else:
            defects = defects + M.defects
        res.append(r)
    if mut is not None:
        return {k2: ([float(x) for x in v] if isinstance(v, list) else float(v)) for k2, v in res[0].items()}
    out = None
    if finite:
        out = {k2: ([Val(a, t) for a, t in zip(v, res[1][k2])] if isinstance(v, list) else Val(v, res[1][k2])) for k2, v in res[0].items()}
    _row_cache[key] = (out, finite, defects)
    return _row_cache[key]


ROW_OUTPUTS = ("W", "rhs", "dw", "rdw", "dW3", "ll_row")


def block_reduce(terms_per_row, n):
    """fp64: a lane's chain over its rows' terms (rows lane, lane + 1024, ..), then the ten-level tree of block_reduce2"""
    s = np.zeros(1024)
    for i in range(n):
        for t in terms_per_row[i]:
            s[i % 1024] += t
    w = 512
    while w >= 1:
        s[:w] += s[w:2 * w]
        w >>= 1
    return float(s[0])


class Reference(object):
    """Everything the entry returns for one case: fp64 restatement, truth (hi + lo) and the two parts of the bound, as arrays in the entry's layout."""

    def __init__(self, case):
        self.case = case
        rows = [eval_row(case, k) for k in range(len(case.templates))]
        self.finite = all(r[1] for r in rows)
        self.defects = [d for r in rows for d in r[2]]
        if not self.finite:
            return
        rt = case.row_t
        self.out = {}
        for name in ROW_OUTPUTS:
            self.out[name] = self._pack([rows[k][0][name] for k in rt])
        self.out["gradF"] = self._pack([v for k in rt for v in rows[k][0]["gradF"]])
        # the one-workgroup reductions: terms in kernel order, Higham's gamma(k) on top of the terms' own bounds
        sums = [("out2_0", "ll_t", case.k_chain + 10), ("out2_1", "q_term", case.k_rows + 10)]
        if HAS_AUX[case.lik]:
            sums += [("out3_0", "e_t", case.k_chain + 10), ("out3_1", "d_t", case.k_chain + 10), ("out3_2", "i_t", case.k_chain + 10)]
        for name, key, kk in sums:
            per_row = [rows[k][0][key] if isinstance(rows[k][0][key], list) else [rows[k][0][key]] for k in rt]
            f64 = block_reduce([[v.f64 for v in r] for r in per_row], case.n)
            flat = [v for r in per_row for v in r]
            tot = MP.fsum([MP.mpf(v.hi) + MP.mpf(v.lo) for v in flat]) if flat else MP.mpf(0)
            hi = to_f64(tot)
            sabs = float(sum(abs(v.hi) for v in flat))
            ea = float(sum(v.ea for v in flat)) + gamma(kk) / U * sabs
            el = np.sum([v.el for v in flat], axis=0) if flat else np.zeros(len(LIB))
            self.out[name] = dict(f64=np.array([f64]), hi=np.array([hi]), lo=np.array([to_f64(tot - MP.mpf(hi))]), ea=np.array([ea]), el=el.reshape(1, -1))

    @staticmethod
    def _pack(vals):
        return dict(f64=np.array([v.f64 for v in vals]), hi=np.array([v.hi for v in vals]), lo=np.array([v.lo for v in vals]),
                    ea=np.array([v.ea for v in vals]), el=np.array([v.el for v in vals]).reshape(len(vals), len(LIB)))

    def ratio(self, name, got, eps):
        """|got - truth| / bound per element (inf where got is not finite); eps: dict f -> eps_f, or a number for all"""
        got = np.asarray(got, dtype=np.float64)
        o = {k: v[:len(got)] for k, v in self.out[name].items()}       # ll_row: the first n_each rows
        ev = np.array([eps[f] if isinstance(eps, dict) else eps for f in LIB], dtype=np.float64)
        bound = U * (o["ea"] + o["el"] @ ev) * (1.0 + 2.0 ** -30)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs((got - o["hi"]) - o["lo"])
            r = np.where(err <= bound, err / np.maximum(bound, 1e-320), np.maximum(err / np.maximum(bound, 1e-320), 1.0 + 2.0 ** -20))
            r = np.where(np.isfinite(got), r, np.inf)
        return r

    def outputs_of_entry(self, res):
        """the entry's result dict (shim.laplace_lik_check) -> name -> array, in this class's names"""
        c = self.case
        d = {k: res[k] for k in ("W", "rhs", "dw", "rdw", "dW3", "gradF")}
        d["ll_row"] = res["ll_each"]
        d["out2_0"], d["out2_1"] = res["out2"][:1], res["out2"][1:2]
        if HAS_AUX[c.lik]:
            for j in range(3):
                d["out3_%d" % j] = res["out3"][j:j + 1]
        return d

    def where(self, name, idx):
        """the grid point behind element idx of an output, for a failure message"""
        c = self.case
        if name.startswith("out"):
            return "sum over %d rows" % c.n
        row = int(np.searchsorted(c.re_ptr, idx, side="right") - 1) if name == "gradF" and c.has_ptr else int(idx)
        tp = c.templates[c.row_t[row]]
        return "row %d: location %r + fixed effect %r, responses %r, weights %r, aux %r, %r" % (row, tp["mode"], tp["fes"][:1] if c.has_fe else None, tp["ys"],
                                                                                              tp["wts"] if c.has_w else None, c.aux, c.aux2)

    def f64_outputs(self):
        return {k: v["f64"] for k, v in self.out.items()}


_ref_cache = {}


def reference(lik, case_idx):
    key = (lik, case_idx)
    if key not in _ref_cache:
        _ref_cache[key] = Reference(Case(lik, *cases(lik)[case_idx]))
    return _ref_cache[key]


# ---- mutants: each must break the bound at eps_f = 16 somewhere on the grid (tests/test_lik_terms_ref.py) ----------------------------------------------------
MUTANTS = (
    ("tetragamma_sign", BETA), ("series_no_u4", PROBIT), ("clamp_1e10", BETA), ("naive_softplus", LOGIT), ("log_for_log1p", PROBIT), ("probit_swap", PROBIT),
    ("trigamma_const", BETA), ("dropped_weight", POISSON), ("no_t3_guard", LOGNORMAL), ("negbin_aux_minus_mu", NEGBIN), ("gamma_single_weight", GAMMA),
)


def mutant_worst(mut, lik, eps=16.0):
    """the worst |mutated fp64 - truth| / bound over the likelihood's cases -> (ratio, output name)"""
    worst = (0.0, None)
    for ci in range(len(cases(lik))):
        ref = reference(lik, ci)
        case = ref.case
        rows = [eval_row(case, k, mut=mut) for k in range(len(case.templates))]
        for name in ROW_OUTPUTS + ("gradF", "out3_0", "out3_1", "out3_2"):
            if name not in ref.out or name.startswith("out2"):
                continue
            if name.startswith("out3"):
                key = {"out3_0": "e_t", "out3_1": "d_t", "out3_2": "i_t"}[name]
                got = [block_reduce([rows[k][key] for k in case.row_t], case.n)]
            elif name == "gradF":
                got = [v for k in case.row_t for v in rows[k]["gradF"]]
            else:
                got = [rows[k][name] for k in case.row_t]
            r = float(np.max(ref.ratio(name, got, eps))) if len(got) else 0.0
            if r > worst[0]:
                worst = (r, name)
    return worst
