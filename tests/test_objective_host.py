"""No GPU: the host side of the objective and optimiser entries (include/sqair_hip.h: sqair_elbo, sqair_elbo_bwd, sqair_rmsprop_step,
sqair_add_l2_grad, sqair_check_finite) -- declared as they were, the ABI version unchanged, the header's paragraphs state what is
refused, and every refusal is made before any HIP call.  Every call here hands over dummy pointers and is one the entry refuses (or
answers, for n = 0 / l2 = 0) before it touches the device; no call with a NULL mean pointer is ever one that is expected to launch."""
import ctypes as C

import pytest

from sqair_amd import _capi
from tests.abi_host import DUMMY, LIBS, constant, err as _err, handle, paragraph, phrases, prototype

D = DUMMY
INT32_MAX = 2147483647


def _means(*ptrs):
    return (C.c_void_p * 8)(*(list(ptrs) + [None] * (8 - len(ptrs))))


def _elbo(lib, h, T=2, B=3, means_in=None, n_means=0, means_out=D, log_w_t=D):
    return lib.sqair_elbo(h, log_w_t, D, T, B, D, D, D, D, D, means_in, n_means, means_out, None)


def test_the_prototypes_and_the_abi_are_unchanged():
    assert prototype("sqair_elbo") == ("int sqair_elbo(SqairHandle* h, const float* log_w_t, const float* disc_lp_t, int T, int B, "
                                       "float* log_weights, float* elbo_iwae_per_example, float* importance_weights, float* vimco_signal, "
                                       "float* scalars_out, const float* const* iw_means_in, int n_means, float* iw_means_out, void* stream)")
    assert prototype("sqair_elbo_bwd") == ("int sqair_elbo_bwd(SqairHandle* h, const float* importance_weights, const float* vimco_signal, "
                                           "int T, int B, float* g_log_w_t, float* g_disc_lp_t, void* stream)")
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    for path in LIBS:
        assert _capi.lib(path).sqair_abi_version() == 2


def test_the_header_states_the_refusals():
    doc = paragraph("Fused IWAE / VIMCO reductions over [T,B,K]", "int sqair_elbo(")
    phrases(doc, ("both may be NULL with n_means = 0 only", "scalars_out[4..15] and iw_means_out[n_means..7] are not written",
                  "k_particles = 1 gives NaN for the VIMCO signal and target",
                  "Refused (return -1, text in sqair_last_error, before any HIP call)", "n_means > 0 with iw_means_in NULL",
                  "a NULL among its first n_means pointers", "with iw_means_out NULL", "T * B * k_particles above 2147483647",
                  "the kernels index with int"))
    doc = paragraph("Gradient of the VIMCO target (already / T)", "int sqair_elbo_bwd(")
    phrases(doc, ("Refused (return -1, text in sqair_last_error, before any HIP call)", "T * B * k_particles above 2147483647"))


@pytest.mark.parametrize("path", LIBS)
def test_elbo_refuses_missing_means_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        for n in (1, 3, 8):
            assert _elbo(lib, h, means_in=None, n_means=n) == -1
            assert _err(lib, h) == "sqair_elbo: iw_means_in must not be NULL with n_means = {}".format(n)
        # a NULL among the first n_means pointers is named by its index; one beyond them is nobody's business
        for n, at in ((1, 0), (3, 1), (3, 2), (8, 7)):
            ptrs = [0x2000 + 0x100 * i for i in range(8)]
            ptrs[at] = None
            assert _elbo(lib, h, means_in=_means(*ptrs), n_means=n) == -1
            assert _err(lib, h) == "sqair_elbo: iw_means_in[{}] must not be NULL with n_means = {}".format(at, n)
        assert _elbo(lib, h, means_in=_means(0x2000, 0x2100, None), n_means=2, means_out=None) == -1
        assert _err(lib, h) == "sqair_elbo: iw_means_out must not be NULL with n_means = 2"        # (index 2 is beyond n_means)
        # the older argument checks come first and say nothing, as before
        before = _err(lib, h)
        assert _elbo(lib, h, n_means=9) == -1 and _elbo(lib, h, n_means=-1) == -1 and _elbo(lib, h, T=0) == -1 and _elbo(lib, h, B=0) == -1
        assert _elbo(lib, h, log_w_t=None, means_in=None, n_means=1) == -1 and _elbo(lib, None) == -1
        assert _err(lib, h) == before


@pytest.mark.parametrize("path", LIBS)
def test_elbo_and_its_adjoint_refuse_more_elements_than_int_indexes(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        for T, B in ((1 << 15, 1 << 15), (1 << 30, 1), (INT32_MAX, 1), (1, INT32_MAX), (INT32_MAX, INT32_MAX)):
            assert T * B * 2 > INT32_MAX
            n = "{} * {} * 2".format(T, B)
            assert _elbo(lib, h, T=T, B=B) == -1
            assert _err(lib, h) == "sqair_elbo: T * B * k_particles = {} must not exceed 2147483647 (the kernels index with int)".format(n)
            assert lib.sqair_elbo_bwd(h, D, D, T, B, D, D, None) == -1
            assert _err(lib, h) == "sqair_elbo_bwd: T * B * k_particles = {} must not exceed 2147483647 (the kernel indexes with int)".format(n)
        # the means are looked at first: the same call with a mean missing names the mean
        assert _elbo(lib, h, T=1 << 15, B=1 << 15, means_in=_means(None), n_means=1) == -1 and "iw_means_in[0]" in _err(lib, h)
        before = _err(lib, h)
        for args in ((None, D, 2, 3, D, D), (D, None, 2, 3, D, D), (D, D, 0, 3, D, D), (D, D, 2, 0, D, D), (D, D, 2, 3, None, D),
                     (D, D, 2, 3, D, None)):
            assert lib.sqair_elbo_bwd(h, args[0], args[1], args[2], args[3], args[4], args[5], None) == -1
        assert lib.sqair_elbo_bwd(None, D, D, 2, 3, D, D, None) == -1 and _err(lib, h) == before


@pytest.mark.parametrize("path", LIBS)
def test_optimiser_and_finite_check_refusals(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        hyper = (1e-3, 0.9, 0.9, 1e-10, 1.0)
        for bad in range(4):
            ptrs = [D, D, D, D]
            ptrs[bad] = None
            assert lib.sqair_rmsprop_step(h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 16, *hyper, None) == -1
        for n in (0, -1, -(1 << 40)):
            assert lib.sqair_rmsprop_step(h, D, D, D, D, n, *hyper, None) == -1
        assert lib.sqair_rmsprop_step(None, D, D, D, D, 16, *hyper, None) == -1
        assert lib.sqair_add_l2_grad(h, None, D, 16, 0.5, None) == -1 and lib.sqair_add_l2_grad(h, D, None, 16, 0.5, None) == -1
        assert lib.sqair_add_l2_grad(h, D, D, -1, 0.5, None) == -1 and lib.sqair_add_l2_grad(None, D, D, 16, 0.5, None) == -1
        # nothing to add: answered before any launch
        assert lib.sqair_add_l2_grad(h, D, D, 0, 0.5, None) == 0 and lib.sqair_add_l2_grad(h, D, D, 16, 0.0, None) == 0
        assert lib.sqair_check_finite(h, None, 16, b"x", D, None) == -1 and lib.sqair_check_finite(h, D, 16, b"x", None, None) == -1
        assert lib.sqair_check_finite(h, D, -1, b"x", D, None) == -1 and lib.sqair_check_finite(None, D, 16, b"x", D, None) == -1
