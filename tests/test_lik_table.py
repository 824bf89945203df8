"""CPU: the likelihood table of the Vecchia-Laplace path (gpboost_amd/csrc/lik_table.h) -- one row per likelihood id -- and the python shim's
name -> (id, num_aux) dict say the same, and the table is plain C++17 that a host compiler takes without HIP (the host-only build of the C API
includes it).  A stand-alone program prints the rows; the ids and names it must print are written out here (they are the ABI of
gpb_hip_vecchia_laplace_set_likelihood)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpboost_amd", "csrc")

NAMES = ["bernoulli_logit", "bernoulli_probit", "poisson", "gamma", "negative_binomial", "beta", "t", "lognormal", "gaussian_latent"]
REAL_ONLY = {"gamma", "beta", "t", "lognormal", "gaussian_latent"}
ALIASES = {"binomial_logit": 0, "binomial_probit": 1, "quasi_bernoulli_logit": 0, "quasi_bernoulli_probit": 1}

PROGRAM = r"""
#include <cstdio>
#include "lik_table.h"
int main(int argc, char** argv) {
  for (int i = 0; i < gpb::kNumLik; ++i)
    std::printf("%d %s %d %d\n", (int)gpb::kLik[i].id, gpb::lik_name(i), gpb::lik_num_aux(i), (int)gpb::lik_real_only(i));
  for (int a = 1; a < argc; ++a) std::printf("%s %d\n", argv[a], gpb::lik_id_of_name(argv[a]));
  return 0;
}
"""


def test_table_rows_match_the_shim_and_the_abi(tmp_path):
    from gpboost_amd import shim
    src, exe = tmp_path / "print_lik_table.cpp", tmp_path / "print_lik_table"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    queries = sorted(ALIASES) + NAMES + ["gaussian", "binomial_", "bernoulli"]
    out = subprocess.check_output([str(exe)] + queries).decode().splitlines()
    rows = [ln.split() for ln in out[:len(NAMES)]]
    assert len(out) == len(NAMES) + len(queries)
    assert [r[1] for r in rows] == NAMES
    assert [int(r[0]) for r in rows] == list(range(9))
    assert {r[1]: (int(r[0]), int(r[2])) for r in rows} == {k: shim._LIKELIHOODS[k] for k in NAMES}
    assert {r[1] for r in rows if int(r[3])} == REAL_ONLY
    resolved = {k: int(v) for k, v in (ln.split() for ln in out[len(NAMES):])}
    assert {k: resolved[k] for k in ALIASES} == ALIASES
    assert {k: shim._LIKELIHOODS[k][0] for k in ALIASES} == ALIASES
    assert set(shim._LIKELIHOODS) == set(NAMES) | set(ALIASES)
    assert [resolved[k] for k in NAMES] == list(range(9))
    assert resolved["gaussian"] == resolved["binomial_"] == resolved["bernoulli"] == -1
