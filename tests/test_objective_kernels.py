"""-m gpu: the objective kernels k_elbo (K <= 64), k_elbo_wide (K > 64) and k_elbo_bwd, each on its own against float64.

They run through the product's entries (sqair_elbo, sqair_elbo_bwd: exactly the launches of a training pass, on caller buffers) and
are compared with tests/objective_ref.py -- the oracle's iwae / vimco_control_variate / vimco / reinforce / ess and the
importance-weighted mean of model.py:202-205 in float64, autograd for the gradients -- pinned on the CPU by
tests/test_objective_ref.py, which also holds the power check over THIS module's case list (objective_ref.CASES / build_case).

Inputs.  Drawn in float64, rounded to float32, the same float32 values to kernel and reference.  Every input array ([T, B K]: the
log-weights, the discrete log-probabilities, eight distinct arrays of means with different content) sits in its own buffer with a
NaN guard row before frame 0 and after frame T - 1; every output sits among distinct sentinel words and is compared bit for bit
outside what the kernel owns -- scalars_out[4..15], iw_means_out[n_means..7] and the buffer of every output passed as NULL included.
Log-weights are drawn per lane and the regimes (objective_ref.REGIMES) are mixed within a batch, so a lane's neighbours in a wave are
in another regime: dominated N(500, 30) per frame; near-equal at large magnitude N(-700, 0.01), ESS ~ K; moderate N(-80, 1); small
N(0, 0.5); two leaders within 0.1 nat with the rest 50 nats below; a lane of bit-equal weights; a lane with one particle 200 nats
below (its float32 weight is exactly 0).  disc_lp is N(-3, 2) per frame with exact zeros, the means N(0, 1) x 10^U(-2, 1).  The
covering list: K 1, 2, 5, 13, 32, 33, 64 | 65, 100, 256, each at T = 1, fpi, fpi + 1, 2 fpi + 3 (fpi = 64 // K frames per load, 1 for
K > 64), B 1, 16, 17, 33, 50, n_means 0, 1, 3, 7, 8, disc_lp_t present and NULL, both vi_target values, each nullable output NULL in
some case with the others still judged, iw_means_in and iw_means_out both NULL in half the n_means = 0 cases; a K = 5 and a K = 100
case also through the wide build.  disc_lp_t, vi_target and the NULL output are dealt with co-prime periods.  The chained test runs
every K 5, 33, 64, 100 case that passes iw and signal: both vi_target values, disc_lp_t NULL, T = 1 among them.  The reference is finite for every
lane drawn (asserted by build_case) but for K = 1 under VIMCO, where signal and scalars[2] are NaN in the reference and must be NaN
from the kernel.  Nothing is selected on a kernel's result, and no element is left out of a comparison.

Metric (objective_ref.scales, from the float64 reference alone).  log_weights / S_bk = sum_t |log_w_t| of the row + log K; signal and
elbo_per_ex / the lane's largest S_bk; elbo_vae, elbo_iwae / the batch's largest; the target / that x (1 + max sum_t |disc_lp_t|) / T;
iw / W_b = max(1, max_k |LW_bk|) -- dw_k = w_k (dLW_k - sum_j w_j dLW_j), |dw| <= max |dLW| / 2: the weights inherit the ABSOLUTE
error of the summed log-weights (3.6e-3 at |LW| ~ 5e4 in the near-equal regime, 7e-8 on this scale; an unscaled bar would be set by
that one case and let everything else through); ess / mean_b W_b ess_b; mean q / mean_b W_b sum_k w_bk mean_t |x_tbk|; chained
g_log_w_t / W_b / (B T), g_disc_lp_t / S_b / (B K T); k_elbo_bwd on its own / the largest reference magnitude of the element's
(frame, lane).  The bar of a (kernel, output) is 8 x the worst error of the float32 restatement of the same formulas over that
kernel's cases (R.bar_from_fp32).  With SQAIR_PARITY_DIR set the figures go to objective_parity.json there
(profiles/objective_parity.json is such a file)."""
import ctypes as C

import numpy as np
import pytest

from tests import kernel_unit as U
from tests import objective_ref as OR
from tests import slot_adjoint_ref as R
from tests.hip_util import stream
from tests.kernel_unit import F64

pytestmark = pytest.mark.gpu

HW, N_SLOTS = (50, 50), 3
CASES = OR.CASES
PARITY = U.Parity(OR.PARITY_FILE, OR.PARITY_NOTE, worst_ratio=True)


def handle(K, wide=False):
    return U.handle("objective K%d%s" % (K, " wide" if wide else ""), lambda name: U.Handle(name, wide, HW, N_SLOTS, K, {}))


_cases = U.Cases(lambda key: {k: OR.build_case(k) for k in CASES} if key == "elbo" else {s: OR.build_bwd_case(s) for s in OR.BWD_SHAPES})


def cases():
    return _cases("elbo")


def worst32(kernel):
    if kernel == "k_elbo_bwd":
        return U.worst32(_cases("bwd"))
    w = OR.worst32(cases(), kernel.split("+")[0])
    chained = kernel.endswith("+k_elbo_bwd")
    return {k: v for k, v in w.items() if k.startswith("g_") == chained}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    U.close()
    PARITY.write(worst32)


def _launch(case, c):
    """One sqair_elbo on fresh buffers: (buffers, {output: what the kernel wrote, float32})."""
    T, B, K, nm = c["T"], c["B"], c["K"], c["n_means"]
    Rw = B * K
    hd = handle(K, c["wide"])
    hd.check(hd.lib.sqair_set_option(hd.h, b"vi_target", c["reinforce"]), "sqair_set_option")
    bufs, ptr = {}, {}
    bufs["log_w_t"], ptr["log_w_t"] = U.pitched(T, Rw, Rw, data=c["lw_t"].reshape(T, Rw))
    if c["dl_t"] is not None:
        bufs["disc_lp_t"], ptr["disc_lp_t"] = U.pitched(T, Rw, Rw, data=c["dl_t"].reshape(T, Rw))
    for q in range(8):
        bufs["x%d" % q], ptr["x%d" % q] = U.pitched(T, Rw, Rw, data=c["xs"][q].reshape(T, Rw))
    at = 0
    for name, width, owned in (("log_weights", Rw, Rw), ("elbo_per_ex", B, B), ("iw", Rw, Rw), ("signal", Rw, Rw), ("scalars", 16, 4),
                               ("means", 8, nm)):
        own = np.arange(width) < (0 if name == c["null"] else owned)
        bufs[name], ptr[name] = U.pitched(1, width, width, out=True, start=at, owned_cols=own)
        at += bufs[name].before.size
    means_in = (C.c_void_p * 8)(*[ptr["x%d" % q] for q in range(8)])
    arg = lambda k: None if k == c["null"] else ptr[k]
    assert nm == 0 or not c["null_means"]                 # (both mean arguments NULL only where the header allows it: n_means = 0)
    hd.check(hd.lib.sqair_elbo(hd.h, ptr["log_w_t"], ptr.get("disc_lp_t"), T, B, arg("log_weights"), arg("elbo_per_ex"), arg("iw"),
                               arg("signal"), arg("scalars"), None if c["null_means"] else means_in, nm,
                               None if c["null_means"] else ptr["means"], stream()), "sqair_elbo")
    for name, b in bufs.items():
        b.check_untouched(name)
    got = {}
    for name, shape in (("log_weights", (B, K)), ("elbo_per_ex", (B,)), ("iw", (B, K)), ("signal", (B, K)), ("scalars", (16,)), ("means", (8,))):
        got[name] = bufs[name].p.view(bufs[name].after()).reshape(shape)
    got["scalars"], got["means"] = got["scalars"][:4], got["means"][:nm]
    return hd, bufs, ptr, got


@pytest.mark.parametrize("case", sorted(CASES))
def test_elbo(case):
    c = cases()[case]
    _, _, _, got = _launch(case, c)
    _, _, _, again = _launch(case, c)
    # the sums run in a fixed order (per-wave partials, then waves in order): a second launch gives the same bits
    for k in c["names"]:
        assert np.array_equal(U.bits(got[k]), U.bits(again[k])), k + " differs between two launches"
    e = OR.errors(got, c["ref"], c["scales"], c["names"])
    assert set(e) == set(c["err32"])
    kernel = OR.kernel_of(case)
    U.judge(PARITY, kernel, case, e, e.get, c["err32"], worst32(kernel))


@pytest.mark.parametrize("case", OR.CHAINED)
def test_elbo_then_elbo_bwd(case):
    """sqair_elbo -> sqair_elbo_bwd against float64 autograd of O.vimco / T (O.reinforce / T)."""
    c = cases()[case]
    T, B, K = c["T"], c["B"], c["K"]
    hd, bufs, ptr, _ = _launch(case, c)
    fwd = {name: bufs[name].after() for name in ("iw", "signal")}
    g = {}
    for i, name in enumerate(("g_log_w_t", "g_disc_lp_t")):
        g[name] = U.pitched(T, B * K, B * K, out=True, start=(1 + i) * (1 << 20))
    hd.check(hd.lib.sqair_elbo_bwd(hd.h, ptr["iw"], ptr["signal"], T, B, g["g_log_w_t"][1], g["g_disc_lp_t"][1], stream()), "sqair_elbo_bwd")
    for name, (b, _) in g.items():
        b.check_untouched(name)
    for name in ("iw", "signal"):                                      # the adjoint's inputs are as sqair_elbo left them
        assert np.array_equal(U.bits(bufs[name].after()), U.bits(fwd[name])), name
    got ={name: b.p.view(b.after()).reshape(T, B, K) for name, (b, _) in g.items()}
    e = OR.errors(got, c["ref"], c["scales"], ["g_log_w_t", "g_disc_lp_t"])
    kernel = OR.kernel_of(case) + "+k_elbo_bwd"
    U.judge(PARITY, kernel, case, e, e.get, c["bwd_err32"], worst32(kernel))


@pytest.mark.parametrize("shape", OR.BWD_SHAPES, ids=lambda s: "T%d B%d K%d" % s)
def test_elbo_bwd(shape):
    """k_elbo_bwd on its own: iw and signal are float32 roundings of the reference's; -iw / (B T) and -sig / (B K T) in float64."""
    c = _cases("bwd")[shape]
    T, B, K = shape
    hd = handle(K)
    iw, sig = U.pitched(1, B * K, B * K, data=c["iw"].reshape(1, -1)), U.pitched(1, B * K, B * K, data=c["sig"].reshape(1, -1))
    g = {name: U.pitched(T, B * K, B * K, out=True, start=i * (1 << 20)) for i, name in enumerate(("g_log_w_t", "g_disc_lp_t"))}
    hd.check(hd.lib.sqair_elbo_bwd(hd.h, iw[1], sig[1], T, B, g["g_log_w_t"][1], g["g_disc_lp_t"][1], stream()), "sqair_elbo_bwd")
    for name, (b, _) in list(g.items()) + [("iw", iw), ("signal", sig)]:
        b.check_untouched(name)
    got = {name: b.p.view(b.after()).reshape(T, B, K).astype(F64) for name, (b, _) in g.items()}
    U.judge(PARITY, "k_elbo_bwd", "T%d B%d K%d" % shape, got, lambda k: R.row_scaled_error(got[k], c["ref"][k]),
            c["err32"], worst32("k_elbo_bwd"))
