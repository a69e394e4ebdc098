"""-m gpu: k_linear_strip (sqair_linear_strip.hip), the one-round kernel of the widest once-per-frame dense launch -- through
sqair_linear_contract_test, the shape selecting the route, and the route asserted for every launch (`fwd_strip`).

The route (sq_launch_linear_strip): a plain-activation layer, 512 <= M < 768 rows, kc < 40, and ceil(mt / 2) x ceil(nt / 6) = 192 ..
256 workgroups -- 55 .. 72 column tiles at 640 rows, 67 .. 90 at 513 and 520.  Everything narrower lost to k_linear when measured
and stays there: the 768-column GRU gate layer (in the pass), the 256- and 400-column layers (isolated); test_strip_leaves_the_gru
pins that, and that the step is still right.

Contract: the rich operand description of tests/test_dense_contract.py (segments with padded pitches, a row divisor, a broadcast
row; an addend on N - 7 columns with its own pitch and divisor; ELU / softplus split; both scales; out_ld = N + 4 and N + 1, the
pad columns NaN before and bit for bit after) against float64 with that file's bar, at the smallest shapes the route takes that
reach each corner: a last row pair holding one live row (M = 513), an odd number of row tiles (520), 640 rows; a strip count that
does not divide the column tiles, with a ragged last tile (N = 1090: 69 tiles, the last strip's second group half empty and its
third empty; N = 887: 56 tiles, the last strip holds 2); kc = 5, 6, 7, 8 and 24 (every kc % 4), 23, and 39 (the deepest before the 32 x 32
tile takes over; its 80 KB image needs the raised LDS limit, which a kc = 35 case -- 72 KB -- asks for first, so that a limit left at
the first launch's size would fail the later ones); 1 .. 4 segments.  One (RT, S, G) is instantiated: (2, 2, 3).

Bits: the strip kernel promises k_linear's result bit for bit (same chunks per wave, same accumulators, same order of the final sum).
One layer on the same buffers at 640 rows (strip) and at 496 rows (split-K, the route asserted): rows 0 .. 495 agree in every bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from tests.hip_util import dev as _dev, stream
from tests.kernel_unit import Fwd, bits as _bits, dense_handle as handle, run_fwd, segments as _segments, took  # noqa: F401  (handle: the module's fixture)

pytestmark = pytest.mark.gpu

# (M, kc, segments, N)
CONTRACT = [
    (640, 35, 2, 1147),   # FIRST: a 72 KB image before the 80 KB ones below (the raised LDS limit is set once per process and kernel)
    (513, 5, 1, 1090),    # the last PAIR of row tiles holds one live row; 12 strips over 69 tiles, ragged last tile
    (520, 6, 2, 1147),    # 33 row tiles, the last workgroup has one
    (640, 7, 3, 1090),    # the rich description itself
    (640, 23, 4, 1147),   # the widest once-per-frame layer's shape
    (520, 39, 2, 1090),   # the deepest K
    (513, 23, 3, 1147),
    (640, 39, 1, 1147),   # the deepest K at 240 workgroups
    (640, 6, 4, 887),     # 10 strips over 56 tiles
    (640, 24, 3, 1090),   # kc % 4 == 0: the four waves hold equal shares, 6 chunks = two whole trips of the K loop
    (520, 8, 1, 1147),    # kc % 4 == 0, 2 chunks per wave: one trip, its third chunk against the zero block
]


@pytest.mark.parametrize("M,kc,nseg,N", CONTRACT)
def test_strip_contract(handle, M, kc, nseg, N):
    L = Fwd(3000 + 7 * kc + M, M, _segments(kc, nseg), N)
    assert L.kc == kc and len(L.segs) == nseg and ((M + 15) // 16) * L.nt > 256
    case = "fwd strip M={} kc={} nseg={} N={}".format(M, kc, nseg, N)
    ref = L.reference(True, M)
    run_fwd(handle, case + " rich out_ld=N+4", L, True, M, 4, "fwd_strip", ref)
    run_fwd(handle, case + " rich out_ld=N+1", L, True, M, 1, "fwd_strip", ref)


def test_strip_leaves_the_gru(handle):
    """One snt.GRU step at 640 rows (x 128 wide, 256 hidden units): the gate layer 640 x 384 x 768 (EPI_GRU1, 160 workgroups in
    strips of 6) and the candidate layer 640 x 256 x 256 (EPI_GRU2) both stay on split-K."""
    lib, h = handle
    M, Kx, nh = 640, 128, 256
    rng = np.random.default_rng(11)
    P, flat = {}, []
    for g in "zrh":
        P["g.w" + g] = (rng.standard_normal((Kx, nh)) / np.sqrt(Kx)).astype(np.float32)
        P["g.u" + g] = (rng.standard_normal((nh, nh)) / np.sqrt(nh)).astype(np.float32)
        P["g.b" + g] = rng.standard_normal(nh).astype(np.float32) * 0.1
        flat += [P["g.w" + g].ravel(), P["g.u" + g].ravel(), P["g.b" + g].ravel()]
    x = rng.standard_normal((M, Kx)).astype(np.float32)
    hs = rng.standard_normal((M, nh)).astype(np.float32)
    out = torch.zeros(M, nh, device="cuda")
    scratch = torch.empty(1 << 23, dtype=torch.float32, device="cuda")
    dx, dh, df = _dev(x), _dev(hs), _dev(np.concatenate(flat))
    before = _capi.dense_routes()
    rc = lib.sqair_gru_test(h, dx.data_ptr(), dh.data_ptr(), df.data_ptr(), out.data_ptr(), M, Kx, scratch.data_ptr(),
                            scratch.numel() * 4, stream())
    assert rc == 0, lib.sqair_last_error(h)
    assert took(before) == {"fwd_splitk": 2}, took(before)
    P64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
    ref = O.gru(P64, "g", torch.tensor(x, dtype=torch.float64), torch.tensor(hs, dtype=torch.float64))
    assert float(np.abs(out.cpu().numpy() - ref.numpy()).max()) < 2e-5


@pytest.mark.parametrize("kc,nseg,N", [(23, 3, 1152), (25, 2, 900)])
def test_strip_does_not_change_a_bit(handle, kc, nseg, N):
    L = Fwd(5000 + kc, 640, _segments(kc, nseg), N)
    assert L.kc == kc
    y_strip = run_fwd(handle, "bits kc={} N={} M=640".format(kc, N), L, True, 640, 4, "fwd_strip")
    y_split = run_fwd(handle, "bits kc={} N={} M=496".format(kc, N), L, True, 496, 4, "fwd_splitk")
    differ = _bits(y_strip[:496]) != _bits(y_split)
    assert not differ.any(), "{} of {} outputs differ between fwd_strip and fwd_splitk".format(int(differ.sum()), differ.size)
