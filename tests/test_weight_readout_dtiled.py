"""Softmax-weight readout of the d-tiled forward (csrc/fa_fwd_dtiled.hip, d = 384 / 512):
fa_fwd_dt_kernel and fa_fwd_dt_kernel<paired>.

The probe, the fp64 reference weights, the gate K eps P + FLOOR, the input families and _State are
those of test_weight_readout.py (read its docstring first; the measured figures of this file are
in its table).  The kernel rounds P to the storage type, sums l by the ones-MFMA and rounds O
once: the steps the bound was derived from, so the bound stands as it is.

What is different here is the geometry: 16 query rows per wave, 64 per workgroup, K and V
streamed through an LDS ring in 32 / 64 / 128-column chunks, and at d = 512 wave pairs (0, 1),
(2, 3) that exchange P^T and, when a wave rescaled, its alpha through LDS: each wave runs P.V for
its own rows and its partner's on its half of the head dim, and the partner's row sums arrive
once at the end.  A selector V maps column c of the probed window to key j0 + c, so "half of the
head dim" is half of the probed keys: a stale partner tile, a missed alpha or a row sum from the
wrong wave shows in the keys j with (j % d) // (d / 2) == h of the rows of one wave.

Lengths (B = 2, H = 2, B * H >= ceil(L / d)): 17 (wave 1 holds one row), 33 (wave 2 one row, its
partner none), 65 (a second workgroup of one row, a tail tile of one key), 130, 256 (no tails),
600 (two probe windows: keys past d are read; ten key tiles, the ring wraps many times).  Chunk
widths (32, 32) and (64, 128) and attention_v1 must give the readout of (128, 128) bit for bit.
Padded head dims 300 (-> 384) and 400 (-> 512): the window is d columns wide, the scale
1 / sqrt(d).

emulate_dtiled_pair emulates one 64-row workgroup of the paired kernel on _State (four waves, 64-key
tiles, P rounded, the partner's P and alpha, the partner's l at the end); without a defect it is
bitwise emulate_forward, as the kernel's paired form is bitwise its unpaired one.  Two defects
are planted in it (test_readout_gate_rejects_pair_defects): the partner's alpha missed on one
tile where a row's maximum rose, and the partner's row sum taken from the wave's own row.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from test_decode import DTYPES, IDS
from test_weight_readout import (LOG2E, TILE, _base2, _exp2_diff, _moving_max_rows, _output_gate_accepts, _State,
                                 _windows, emulate_forward, fwd_inputs, fwd_weights, read_all, readout_check,
                                 readout_gate)

FAMILIES = ("flat", "steep")  # full attention has no forbidden key: no tempt
B, H = 2, 2
HEAD_DIMS = (384, 512)
LENGTHS = (17, 33, 65, 130, 256, 600)
PADDED = ((300, 384), (400, 512))  # (d, the kernel's head dim) at L = 130, bf16
PAD_L = 130
CHUNKS = ((32, 32), (64, 128))  # (d_tile_qk, d_tile_v) that must reproduce (128, 128) bit for bit
ROWS = 64  # query rows of a workgroup: four waves of 16
EMU_L = (130, 600)


@functools.lru_cache(maxsize=None)
def _case(family, L_, d, dtype):
    """(q, k, P, vis, s) of a case, shared by the tests and left unchanged."""
    q, k = fwd_inputs(family, B, H, H, L_, d, dtype)
    P, vis, s = fwd_weights(q, k, False)
    for x in (P, s):
        x.setflags(write=False)
    return q, k, P, vis, s


def _label(d, L_):
    """What the library reports for one d-tiled launch at kernel head dim d."""
    return f"{'fa_fwd_dt_kernel<paired>' if d == 512 else 'fa_fwd_dt_kernel'} [grid {B * H * -(-L_ // ROWS)}]"


# ----------------------------------------------------------------------------------------
# the emulation of one paired workgroup
# ----------------------------------------------------------------------------------------


def emulate_dtiled_pair(s2, d, dtype, skip_alpha=None, own_sum=None):
    """One 64-row workgroup of fa_fwd_dt_kernel<paired>: s2 [R <= 64, n] base-2 scores.  Wave w
    owns rows 16 w .. 16 w + 15 (fewer, or none, at the end of a sequence) and the column half
    hh = w & 1, the keys j with (j % d) // (d / 2) == hh under a selector V.  Per 64-key tile every
    wave folds its own rows (P rounded to the storage type, l from the rounded P) and hands P and
    alpha to its partner w ^ 1; it accumulates its own rows (o) and the partner's (op) on its
    half, the partner's with the partner's alpha; at the end the partner's l normalises op.
    Row i of wave w is therefore o of wave w on half hh and op of wave w ^ 1 on the other half.

    Defects: skip_alpha = (w, t, rows): wave w does not apply its partner's alpha of tile t to
    the rows `rows` (indices inside the partner's block) of op; own_sum = w: wave w normalises op
    by its own l of the same row index.  Returns (weights fp32, output storage tensor)."""
    R, n = s2.shape
    blocks = [slice(min(16 * w, R), min(16 * w + 16, R)) for w in range(4)]
    half = (np.arange(n) % d) // (d // 2)
    st = [_State(b.stop - b.start, n) for b in blocks]
    op = [np.zeros((blocks[w ^ 1].stop - blocks[w ^ 1].start, n), np.float32) for w in range(4)]
    for t, t0 in enumerate(range(0, n, TILE)):
        cols = slice(t0, min(t0 + TILE, n))
        alpha, p = [], []
        for w in range(4):
            m_old = st[w].m.copy()
            st[w].fold(s2[blocks[w]], cols, dtype)  # o *= alpha, o[:, cols] = P, l = l alpha + sum P
            alpha.append(_exp2_diff(m_old, st[w].m))
            p.append(st[w].acc[:, cols].copy())
        for w in range(4):
            a = alpha[w ^ 1].copy()
            if skip_alpha is not None and skip_alpha[:2] == (w, t):
                a[skip_alpha[2]] = 1
            op[w] *= a[:, None]
            op[w][:, cols] = p[w ^ 1]
    out = np.zeros((R, n), np.float32)
    for w in range(4):
        mine = half == (w & 1)
        own = st[w].normalised()
        out[blocks[w]][:, mine] = own[:, mine]
        lp = st[w ^ 1].l
        if own_sum == w:  # rows the wave does not have keep the partner's sum
            lp = lp.copy()
            k_ = min(len(lp), len(st[w].l))
            lp[:k_] = st[w].l[:k_]
        out[blocks[w ^ 1]][:, mine] = (op[w] * (np.float32(1) / lp)[:, None])[:, mine]
    return out, torch.from_numpy(out).to(dtype)


def emulate_dtiled_case(s, d, dtype, defect_at=None, **defect):
    """emulate_dtiled_pair over every workgroup of natural fp64 scores s [B, H, L, L]; the defect,
    if any, in workgroup defect_at = (b, h, qt) only."""
    w = np.zeros(s.shape, np.float32)
    s2 = _base2(s, np.ones(s.shape, bool), d)
    for b, h, r0 in itertools.product(range(s.shape[0]), range(s.shape[1]), range(0, s.shape[2], ROWS)):
        kw = defect if defect_at == (b, h, r0 // ROWS) else {}
        w[b, h, r0:r0 + ROWS] = emulate_dtiled_pair(s2[b, h, r0:r0 + ROWS], d, dtype, **kw)[0]
    return w, torch.from_numpy(w).to(dtype)


# ----------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------


def test_dtiled_input_families_have_their_properties():
    """Per case actually used: steep rows span at most 40 log2 units (bf16 never meets its floor)
    and, from L = 130 on, the row maximum moves between 64-key tiles in at least a third of the
    rows; every flat weight lies within e^(+-8) of 1 / L."""
    cases = [(d, L_, dt) for d, L_, dt in itertools.product(HEAD_DIMS, LENGTHS, DTYPES)]
    cases += [(d, PAD_L, torch.bfloat16) for d, _ in PADDED]
    seen = {}
    for d, L_, dtype in cases:
        assert B * H >= _windows(L_, d)  # every rotation touches every window
        _, _, P, vis, s = _case("flat", L_, d, dtype)
        assert np.isfinite(s).all()
        off = float(np.abs(np.log(P * L_)).max())
        assert off < 8, (d, L_, IDS[dtype], off)
        _, _, _, vis, s = _case("steep", L_, d, dtype)
        assert np.isfinite(s).all() and np.abs(s).max() < 1e3
        span = float((s.max(-1) - s.min(-1)).max()) * LOG2E
        assert span <= 40, (d, L_, IDS[dtype], span)
        moved = float(_moving_max_rows(s, vis).mean())
        if L_ >= 130:
            assert moved >= 1 / 3, (d, L_, IDS[dtype], moved)
        seen[d, L_, IDS[dtype]] = (round(span, 1), round(off, 1), round(moved, 2))
    print("d-tiled cases (steep span in log2 units, flat |log(P L)|, steep rows with a moving maximum):", seen)


@pytest.mark.parametrize("d", (300, 512))
def test_dtiled_probe_reads_the_reference(d):
    """The probe's plumbing on the CPU: with the fp64 reference in the kernel's place (rounded
    once) every weight comes back inside the bound -- two windows at L = 600, the window of a
    padded head dim d columns wide."""
    dtype, L_ = torch.bfloat16, 600 if d == 512 else PAD_L
    q, k, P, vis, _ = _case("flat", L_, d, dtype)
    got = read_all(lambda v: torch.from_numpy(P @ v.double().numpy()).to(dtype), B, H, H, L_, L_, d, dtype)
    assert got.shape[-1] == _windows(L_, d) * d
    assert readout_gate(got, P, vis, dtype, f"probe d={d}", quiet=True) <= 0.26  # one rounding


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("family", FAMILIES)
def test_dtiled_emulation_stays_inside_the_bound(family, dtype):
    """The paired workgroup's steps, emulated: at most 0.75 of K eps P + FLOOR, and bitwise the
    unpaired order of the same steps (emulate_forward), as the kernel's two forms are."""
    worst = {}
    for L_, d in itertools.product(EMU_L, HEAD_DIMS):
        _, _, P, vis, s = _case(family, L_, d, dtype)
        plain = emulate_forward(_base2(s, vis, d).reshape(-1, L_), dtype)[1].reshape(P.shape)
        worst[f"d{d} L{L_}"] = readout_gate(plain, P, vis, dtype, "emulation d-tiled", limit=0.75, quiet=True)
        if d == 512:
            out = emulate_dtiled_case(s, d, dtype)[1]
            assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), (L_, d)
    print(f"emulation d-tiled {family} {IDS[dtype]}:", {k_: round(v, 3) for k_, v in worst.items()})


def _rise(s2, rows):
    """(rise in base-2 units, tile, row) of the largest rise of a row's running maximum at a tile
    t >= 1, among `rows`."""
    best = (0.0, None, None)
    for i in rows:
        run = s2[i, :TILE].max()
        for t in range(1, -(-s2.shape[1] // TILE)):
            mx = s2[i, t * TILE:(t + 1) * TILE].max()
            if mx - run > best[0]:
                best = (float(mx - run), t, i)
            run = max(run, mx)
    return best


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_readout_gate_rejects_pair_defects(dtype):
    """Two defects of the wave pairs, planted in workgroup 0 of head (0, 0) at d = 512, L = 600:
    the readout gate rejects each; what the output gate (A + eps |ref| on P @ V, V ~ N(0, 1))
    says to the same weights is printed."""
    d, L_ = 512, 600

    def rejected(P, vis, out):
        leaked, bad, worst = readout_check(out, P, vis, dtype)
        return leaked > 0 or bad > 0 or worst > 1.0, (leaked, bad, round(worst, 2))

    for family in FAMILIES:  # the clean emulation passes both gates
        _, _, P, vis, s = _case(family, L_, d, dtype)
        w, out = emulate_dtiled_case(s, d, dtype)
        assert not rejected(P, vis, out)[0] and _output_gate_accepts(w, P, dtype, 11)

    # 1. wave 0 holds the rows of wave 1 (16..31) on half 0 (keys 0..255 and 512..599): on the tile
    # where one of them rose most it misses wave 1's alpha -- in all 16 rows, then in that row alone
    _, _, P, vis, s = _case("steep", L_, d, dtype)
    s2 = _base2(s, vis, d)[0, 0, :ROWS]
    rise, t, i = _rise(s2, range(16, 32))  # (the keys before any tile t >= 1 include 0..63, of half 0)
    assert rise >= 1 and t >= 1, (rise, t)  # alpha <= 1 / 2
    for rows, what in ((slice(None), "every row of the wave"), ([i - 16], f"row {i} alone")):
        w, out = emulate_dtiled_case(s, d, dtype, defect_at=(0, 0, 0), skip_alpha=(0, t, rows))
        r, why = rejected(P, vis, out)
        assert r, (what, why)
        # only rows of wave 1 and keys of half 0 before tile t may differ from the clean run
        clean = emulate_dtiled_case(s, d, dtype)[0]
        diff = np.argwhere(w != clean)
        assert len(diff) and (diff[:, :2] == 0).all() and ((diff[:, 2] >= 16) & (diff[:, 2] < 32)).all()
        assert (diff[:, 3] < t * TILE).all() and ((diff[:, 3] % d) < d // 2).all()
        print(f"missed partner alpha (tile {t}, rise 2^{rise:.1f}), {what}: readout", why, "output gate accepts:",
              _output_gate_accepts(w, P, dtype, 11))

    # 2. wave 0 normalises wave 1's rows by its own row sums (flat family, the pair (0, 1))
    _, _, P, vis, s = _case("flat", L_, d, dtype)
    w, out = emulate_dtiled_case(s, d, dtype, defect_at=(0, 0, 0), own_sum=0)
    r, why = rejected(P, vis, out)
    assert r, why
    print("partner's row sum from the wave's own row: readout", why, "output gate accepts:",
          _output_gate_accepts(w, P, dtype, 11))


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("L_", LENGTHS, ids=lambda x: f"L{x}")
@pytest.mark.parametrize("d", HEAD_DIMS, ids=lambda x: f"d{x}")
def test_readout_dtiled(gpu, d, L_, dtype, family):
    from exploring_flash_attention_amd import ops
    nw = _windows(L_, d)
    assert B * H >= nw
    q, k, P, vis, _ = _case(family, L_, d, dtype)
    qd, kd = q.to(gpu), k.to(gpu)
    with ops.launched_kernels() as kl:
        got = read_all(lambda v: ops.attention_tiled_d(qd, kd, v.to(gpu), 128, 128), B, H, H, L_, L_, d, dtype)
    assert kl == [_label(d, L_)] * nw, kl
    readout_gate(got, P, vis, dtype, f"op=dtiled dtype={IDS[dtype]} family={family} d={d} L={L_}")
    for dq, dv in CHUNKS:  # the chunking changes the schedule, not the sums
        with ops.launched_kernels() as kl:
            other = read_all(lambda v: ops.attention_tiled_d(qd, kd, v.to(gpu), dq, dv), B, H, H, L_, L_, d, dtype)
        assert kl == [_label(d, L_)] * nw, kl
        assert torch.equal(_bits(other), _bits(got)), (dq, dv)
    with ops.launched_kernels() as kl:
        other = read_all(lambda v: ops.attention_v1(qd, kd, v.to(gpu)), B, H, H, L_, L_, d, dtype)
    assert kl == [_label(d, L_)] * nw, kl
    assert torch.equal(_bits(other), _bits(got)), "attention_v1"


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,D", PADDED, ids=[f"d{d}" for d, _ in PADDED])
def test_readout_dtiled_padded_head_dim(gpu, d, D, family):
    """d = 300 / 400 zero-padded to 384 / 512: the window is d columns wide, the scale 1 / sqrt(d);
    the padding columns never reach the caller (read_all asserts the output's shape and dtype)."""
    from exploring_flash_attention_amd import ops
    dtype, L_ = torch.bfloat16, PAD_L
    assert ops.kernel_head_dim(d) == D
    q, k, P, vis, _ = _case(family, L_, d, dtype)
    qd, kd = q.to(gpu), k.to(gpu)

    def call(v):
        out = ops.attention_tiled_d(qd, kd, v.to(gpu), 128, 128)
        assert out.dtype == dtype and tuple(out.shape) == (B, H, L_, d)
        return out

    with ops.launched_kernels() as kl:
        got = read_all(call, B, H, H, L_, L_, d, dtype)
    assert kl == [_label(D, L_)] * _windows(L_, d), kl
    readout_gate(got, P, vis, dtype, f"op=dtiled-padded dtype={IDS[dtype]} family={family} d={d}->{D} L={L_}")
