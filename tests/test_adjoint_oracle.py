"""The numpy statement of the gradient's adjoint (tests/adjoint_ref.py) against the forward operator: the transpose of the
dense matrix built from np_gradients, and the dot-product identity <g, gbar> = <var, A^T gbar> against the COMPILED
reference's golden gradients -- which ties the adjoint to the reference's own forward operator.  CPU only."""
import glob
import os

import numpy as np
import pytest

from adjoint_ref import dense_gradient_matrix, np_adjoint_scale, np_gradients_adjoint
from conftest import GOLDEN, ROOT, load_golden

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def fixture_domains(fx):
    nd = int(fx["ndomains"])
    for d in range(nd):
        if f"d{d}_fpoint" in fx.files:
            yield d, fx[f"d{d}_fpoint"], fx[f"d{d}_fnormal"], fx[f"d{d}_pvolume"], int(fx[f"d{d}_nown"]), fx[f"d{d}_var"]


@pytest.mark.parametrize("name", FIXTURES)
def test_np_adjoint_is_the_dense_transpose(orc, name):
    fx = load_golden(name)
    rng = np.random.default_rng(sum(name.encode()))
    for d, fp, fn, vol, nown, _ in list(fixture_domains(fx))[:2]:
        nall = len(vol)
        A = dense_gradient_matrix(orc.np_gradients, fp, fn, vol, nown)
        gbar = rng.standard_normal((nall, 7, 3))
        want = (A.T @ gbar[:nown].ravel()).reshape(nall, 7)
        got = np_gradients_adjoint(fp, fn, vol, gbar, nown)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), (name, d)
        # ghost rows of gbar do not enter (ghosts = False)
        g2 = gbar.copy()
        g2[nown:] = 1e30
        assert np.array_equal(np_gradients_adjoint(fp, fn, vol, g2, nown), got)


@pytest.mark.parametrize("name", FIXTURES)
def test_dot_product_identity_against_compiled_reference_gradients(name):
    """<g_ref, gbar> over the owned rows == <var, A^T gbar> over every row, g_ref = the compiled reference's gradients of
    the fixture (its var, ghost rows included: the reference's forward map is affine in them)"""
    fx = load_golden(name)
    rng = np.random.default_rng(7)
    checked = 0
    for d, fp, fn, vol, nown, var in fixture_domains(fx):
        for key in [k for k in fx.files if k.startswith("grad_") and k.endswith(f"_d{d}")]:
            g_ref = fx[key]
            gbar = rng.standard_normal(g_ref.shape)
            vbar = np_gradients_adjoint(fp, fn, vol, gbar, nown)
            lhs_terms = g_ref[:nown] * gbar[:nown]
            rhs_terms = var * vbar
            lhs, rhs = lhs_terms.sum(), rhs_terms.sum()
            bound = 1e-12 * max(np.abs(lhs_terms).sum(), np.abs(rhs_terms).sum())
            assert abs(lhs - rhs) <= bound, (name, key, lhs, rhs)
            checked += 1
    assert checked > 0, name


def test_adjoint_scale_bounds_the_adjoint():
    rng = np.random.default_rng(3)
    fp = rng.integers(0, 40, (200, 2)).astype(np.int32)
    fn, vol, gbar = rng.standard_normal((200, 3)), rng.uniform(0.5, 2, 40), rng.standard_normal((40, 7, 3))
    v = np_gradients_adjoint(fp, fn, vol, gbar, 30)
    s = np_adjoint_scale(fp, fn, vol, gbar, 30)
    assert np.all(np.abs(v) <= s * (1 + 1e-12))


def test_adjoint_entry_points_are_declared(pkg):
    from test_abi_symbols import declared_functions
    hip = declared_functions("cfdproxy_hip.h")
    for n in ("cfdp_gpu_set_grad_adjoint", "cfdp_gpu_get_var_adjoint", "cfdp_gpu_gradients_adjoint", "cfdp_gpu_adjoint_group",
              "cfdp_gpu_step_adjoint_rccl", "cfdp_gpu_adjoint_ptrs"):
        assert n in hip, n
        assert hasattr(pkg.hip_lib(), n), n


def test_algo_bytes_adjoint(pkg):
    assert pkg.algo_bytes_adjoint(10, 4, 2) == 32 * 10 + 232 * 4 + 176 * 2
    # per owned point: the forward's var row (64) + grad row (168) become the adjoint's gbar row + 1/V (176) + vbar row (56)
    assert pkg.algo_bytes_adjoint(0, 1, 0) == pkg.algo_bytes_grad(0, 1, 0)
