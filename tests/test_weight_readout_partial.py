"""Softmax-weight readout of the row-layout partial kernels and the stand-alone combine, the
building blocks of the multi-GPU path: fa_fwd_kernel<partial>, fa_fwd16_kernel<partial>, their
strided forms (row-range views of q), and fa_combine_kernel in its three partial formats.

The probe, the fp64 reference weights, the gate K eps P + FLOOR, split_extra, the input families
and _State are those of test_weight_readout.py (read its docstring first; the measured figures of
this file are in its table).  What this file adds:

Shards.  Shard s holds the keys [s kps, min((s + 1) kps, Lk)) as contiguous copies of K and of
the selector V, and runs through ops.attention_partial in the chunk layout of the multi-GPU
exchange ([Lq / chunk_rows, B * H, chunk_rows, d]); every key window of d keys is probed by
rotation over (b, h), so every key of every shard is read, and every column of a probed window
outside the shard must read bitwise +-0.

The raw partial, decoded (scaled: an exact ldexp by the stored e; the chunk layout undone), is
gated against the shard-local fp64 weights P_loc, the softmax over the shard's keys only:
  fp32 partials    (K - 1) eps P_loc + FLOOR: the bound's derivation less the output's half-ulp,
                   which an fp32 store does not have;
  input type       K eps P_loc + FLOOR: rounded once, like an output;
  scaled fp16      (K - 1) eps P_loc + FLOOR + split_extra(P_loc, d, kps, "scaled"): eps of the
                   storage type (P is still rounded to it before P.V), the fp16 store's own
                   half-ulp 2^-11 is at most one of K's spare eps, its subnormal spacing the
                   derived term.
The lse is gated against the fp64 base-2 lse of the shard (scores times log2 e / sqrt(d)):
  |lse - ref| <= K eps log2(e) + 2^-21 max(1, |ref|)
(l is summed from P values of at most a relative half-ulp eps each, so log2 l moves by at most
eps log2 e, K the same margin factor; the second term: fp32 m and scores), and for scaled
partials e is an integer with the decoded row maximum in [0.5, 1] 2^e.  ops.combine of all
shards' partials is gated against the full-row weights with K eps P + FLOOR + split_extra(P, d,
kps, fmt): the fused split-KV tests' bound, the same formats and combine arithmetic.

emulate_partial_combine holds emulate_v2's steps (per-shard _State, format rounding, {lse, e},
the base-2 combine in shard order, a ragged last shard) to 0.75 of each of those bounds, and
carries two defects (test_readout_gate_rejects_partial_defects): the last key of the last shard
dropped in the last row of each chunk, and the combine applying row r's exponent e to row r ^ 1.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from test_decode import DTYPES, GATE, IDS
from test_weight_readout import (K_ULP, LOG2E, PARTIAL_FORMATS, _base2, _exp2_diff, _gen, _output_gate_accepts,
                                 _round_to, _scores, _softmax, _State, _windows, readout_check, readout_gate,
                                 selector, split_extra)

FAMILIES = ("flat", "steep")
B, H = 2, 2
# (d, Lq, chunk_rows, Lk, keys per shard)
CASES = ((64, 200, 50, 193, 64),     # fa_fwd_kernel<partial>; chunks straddle the 128-row query tile; last shard one key
         (128, 200, 100, 193, 64),   # d = 128 (whole-tile shards: fa_fwd16_kernel<partial>), the key tail: fa_fwd_kernel
         (128, 256, 64, 256, 64),    # fa_fwd16_kernel<partial>, whole tiles
         (128, 256, 64, 256, 128),   # the same kernel, two tiles per shard
         (32, 200, 200, 193, 96),    # a shard tail of one key
         (256, 96, 32, 97, 32))      # 32-key tiles, last shard one key
STRIDED_CASE = (128, 256, 64, 193, 64)  # shards of 64, 64, 64 and 1 keys: both strided kernels
CASE_IDS = ["d%d-Lq%d-cr%d-Lk%d-kps%d" % c for c in CASES]
EMU_CASES = (CASES[0], CASES[-1])


def _pdtype(fmt, dtype):
    from exploring_flash_attention_amd import ops
    return {"fp32": torch.float32, "input": dtype, "scaled": ops.PARTIAL_FP16_SCALED}[fmt]


def _tile(d):
    return 64 if d <= 128 else 32  # keys per tile of the forward kernels


@functools.lru_cache(maxsize=None)
def partial_inputs(family, B, H, Lq, Lk, d, dtype):
    """Storage-rounded q [B, H, Lq, d], k [B, H, Lk, d] of a partial case; nobody writes to them."""
    g = _gen("partial", family, B, H, Lq, Lk, d)
    q = torch.randn(B, H, Lq, d, generator=g) * {"flat": 1.0, "steep": 3.0}[family]
    k = torch.randn(B, H, Lk, d, generator=g)
    return q.to(dtype), k.to(dtype)


def _shards(Lk, kps):
    return [(k0, min(k0 + kps, Lk)) for k0 in range(0, Lk, kps)]


@functools.lru_cache(maxsize=None)
def _case(family, case, dtype):
    """(q, k, s, P): fp64 natural scores and full-row weights [B, H, Lq, Lk], left unchanged."""
    d, Lq, _, Lk, _ = case
    q, k = partial_inputs(family, B, H, Lq, Lk, d, dtype)
    s = _scores(q, k)
    P = _softmax(s, np.ones(s.shape, bool))
    for x in (s, P):
        x.setflags(write=False)
    return q, k, s, P


def shard_weights(s, k0, k1):
    """(P_loc, vis, lse2) of the shard [k0, k1): the softmax over its keys only, zero elsewhere
    [B, H, Lq, Lk]; vis marks its columns; lse2 [B, H, Lq] its fp64 base-2 log-sum-exp."""
    vis = np.zeros(s.shape, bool)
    vis[..., k0:k1] = True
    s2 = s[..., k0:k1] * LOG2E
    mx = s2.max(-1)
    return _softmax(s, vis), vis, mx + np.log2(np.exp2(s2 - mx[..., None]).sum(-1))


def partial_bound(fmt):
    """(k_ulp, whether split_extra's scaled term is added) of the raw partial's gate."""
    return {"fp32": (K_ULP - 1, False), "input": (K_ULP, False), "scaled": (K_ULP - 1, True)}[fmt]


def lse_bound(ref, dtype):
    return K_ULP * GATE[dtype][2] * LOG2E + 2.0 ** -21 * np.maximum(1.0, np.abs(ref))


# ----------------------------------------------------------------------------------------
# the probe: shards through a partial function, their partials through a combine function
# ----------------------------------------------------------------------------------------


def unchunk(x, B, H):
    """[Lq / cr, B * H, cr, ...] -> [B, H, Lq, ...]."""
    nch, BH, cr = x.shape[:3]
    return x.transpose(0, 1).reshape((B, H, nch * cr) + tuple(x.shape[3:]))


def decode_partial(o_part, lse, fmt, dtype):
    """(partial [B, H, Lq, d] -- fp32, or the input type as stored --, lse [B, H, Lq] fp32, e or
    None) of what a partial launch wrote, on the host.  Scaled: e is an integer, every nonzero
    row's largest stored value lies in [0.5, 1], and the decoding is an exact ldexp."""
    o_part, lse = unchunk(o_part.cpu(), B, H), unchunk(lse.cpu(), B, H)
    assert lse.dtype == torch.float32
    if fmt != "scaled":
        assert o_part.dtype == (torch.float32 if fmt == "fp32" else dtype) and lse.dim() == 3
        return o_part.contiguous(), lse.contiguous(), None
    assert o_part.dtype == torch.float16 and lse.shape[-1] == 2
    e = lse[..., 1]
    assert torch.equal(e, e.round()), "e is not an integer"
    rmax = o_part.float().abs().amax(-1)
    assert bool((((rmax >= 0.5) & (rmax <= 1.0)) | (rmax == 0)).all()), "a row maximum outside [0.5, 1] 2^e"
    return torch.ldexp(o_part.float(), e[..., None]).contiguous(), lse[..., 0].contiguous(), e.contiguous()


def _place(dst, out, r, nw, d):
    """What rotation r read, put in key order (read_all's placement, H_kv == H)."""
    for n in range(B * H):
        w = (n + r) % nw
        dst[n // H, n % H, :, w * d:(w + 1) * d] = out[n // H, n % H]


def read_partials(partial, combine, case, q, k, fmt, dtype, dev="cpu"):
    """Every rotation of the selector through every shard and the combine.  partial(q, k_s, v_s,
    chunk_rows, fmt) -> (o_part, lse) as ops.attention_partial; combine(o_parts [S, B*H, Lq, d],
    lses, fmt) -> [B, H, Lq, d].  Returns (raw [S] of [B, H, Lq, windows * d] decoded partials,
    lse [S] of [B, H, Lq], combined [B, H, Lq, windows * d] storage type)."""
    d, Lq, cr, Lk, kps = case
    nw, sh = _windows(Lk, d), _shards(Lk, kps)
    qd = q.to(dev)
    ks = [k[:, :, k0:k1].contiguous().to(dev) for k0, k1 in sh]
    raw = [torch.full((B, H, Lq, nw * d), float("nan"), dtype=dtype if fmt == "input" else torch.float32) for _ in sh]
    comb = torch.full((B, H, Lq, nw * d), float("nan"), dtype=dtype)
    lses = None
    for r in range(nw):
        v = selector(B, H, Lk, d, r, dtype)
        parts = [partial(qd, ks[i], v[:, :, k0:k1].contiguous().to(dev), cr, fmt) for i, (k0, k1) in enumerate(sh)]
        dec = [decode_partial(o, l, fmt, dtype) for o, l in parts]
        for i, (o, _, _) in enumerate(dec):
            _place(raw[i], o, r, nw, d)
        if lses is None:
            lses = [l for _, l, _ in dec]
        else:  # the lse does not depend on V
            assert all(torch.equal(l.view(torch.int32), l0.view(torch.int32)) for (_, l, _), l0 in zip(dec, lses))
        o_all = torch.stack([unchunk(o, B, H).reshape(B * H, Lq, d) for o, _ in parts]).contiguous()
        l_all = torch.stack([unchunk(l, B, H).reshape((B * H, Lq) + tuple(l.shape[3:])) for _, l in parts]).contiguous()
        out = combine(o_all, l_all, fmt).cpu()
        assert out.dtype == dtype and tuple(out.shape) == (B, H, Lq, d)
        _place(comb, out, r, nw, d)
    return raw, lses, comb


def gate_partials(raw, lses, comb, case, s, P, fmt, dtype, label, limit=1.0):
    """The three gates of this file; the worst err / bound of each: (raw, lse, combine)."""
    d, _, _, Lk, kps = case
    k_ulp, scaled = partial_bound(fmt)
    w_raw = w_lse = 0.0
    for i, (k0, k1) in enumerate(_shards(Lk, kps)):
        P_loc, vis, lse_ref = shard_weights(s, k0, k1)
        w_raw = max(w_raw, readout_gate(raw[i], P_loc, vis, dtype, f"{label} raw shard {i}", limit=limit, quiet=True,
                                        extra=split_extra(P_loc, d, kps, "scaled", dtype) if scaled else None,
                                        k_ulp=k_ulp))
        got = lses[i].double().numpy()
        assert np.isfinite(got).all(), (label, i)
        w_lse = max(w_lse, float((np.abs(got - lse_ref) / lse_bound(lse_ref, dtype)).max()))
    assert w_lse <= limit, (label, "lse", w_lse)
    w_comb = readout_gate(comb, P, np.ones(P.shape, bool), dtype, f"{label} combine", limit=limit, quiet=True,
                          extra=split_extra(P, d, kps, fmt, dtype))
    return w_raw, w_lse, w_comb


# ----------------------------------------------------------------------------------------
# the fp64 reference in the kernels' place, and the emulation
# ----------------------------------------------------------------------------------------


def _encode(x, lse2, cr, fmt, dtype):
    """fp64 partial x [B, H, Lq, d] and base-2 lse [B, H, Lq] in a partial launch's layout and
    format (scaled: e the exponent of the row's largest value, as frexp gives it)."""
    Lq, d = x.shape[2:]
    chunk = lambda t: t.reshape((B * H, Lq // cr, cr) + tuple(t.shape[3:])).transpose(0, 1).contiguous()
    x, lse = torch.from_numpy(x), torch.from_numpy(lse2).float()
    if fmt == "scaled":
        e = torch.frexp(x.abs().amax(-1).float())[1]
        return chunk(torch.ldexp(x, -e[..., None].double()).half()), chunk(torch.stack([lse, e.float()], -1))
    return chunk(x.to(torch.float32 if fmt == "fp32" else dtype)), chunk(lse)


def ref_partial(q, k_s, v_s, cr, fmt):
    s = _scores(q, k_s)
    P = _softmax(s, np.ones(s.shape, bool))
    s2 = s * LOG2E
    mx = s2.max(-1)
    return _encode(P @ v_s.double().numpy(), mx + np.log2(np.exp2(s2 - mx[..., None]).sum(-1)), cr, fmt, q.dtype)


def ref_combine(o_all, l_all, fmt, dtype):
    """fp64 combine of [S, B*H, Lq, d] partials with base-2 lse ({lse, e} for scaled ones)."""
    o = o_all.double()
    if fmt == "scaled":
        o, l_all = torch.ldexp(o, l_all[..., 1:].double()), l_all[..., 0]
    w = torch.exp2(l_all.double() - l_all.double().amax(0))
    out = (w[..., None] * o).sum(0) / w.sum(0)[..., None]
    return out.reshape((B, H) + tuple(out.shape[1:])).to(dtype)


def emulate_partial_combine(s2, d, kps, fmt, dtype, drop_rows=None, swap_e=False):
    """The steps of attention_partial per shard and of the combine, on rows s2 [R, Lk] of base-2
    scores, as emulate_v2 takes them: per shard of kps keys (the last one ragged) the forward's
    key tiles (64 keys, 32 at d = 256; P rounded, l from the rounded P), the normalised partial
    rounded to the format -- scaled: per probed window of d keys, what one launch's row holds,
    times 2^-e to fp16 --, {lse, e}, and the base-2 combine in shard order.

    Defects: drop_rows (a boolean [R]): those rows do not see the last key of the last shard;
    swap_e: the combine decodes row r with the exponent of row r ^ 1.
    Returns (decoded partials [S] of [R, Lk] -- fp32, or storage tensors for the input type --,
    lse [S] of [R] fp32, combined weights fp32 [R, Lk], the output as a storage tensor)."""
    R, Lk = s2.shape
    tile = _tile(d)
    if drop_rows is not None:
        s2 = s2.copy()
        s2[drop_rows, Lk - 1] = -np.inf
    parts, seen, lses = [], [], []
    for k0, k1 in _shards(Lk, kps):
        st = _State(R, Lk)
        for t0 in range(k0, k1, tile):
            st.fold(s2, slice(t0, min(t0 + tile, k1)), dtype)
        part = st.normalised()
        used = part  # what the combine decodes
        if fmt == "input":
            part = used = _round_to(part, dtype)
        elif fmt == "scaled":
            used = part.copy()
            for w0 in range(0, Lk, d):
                cols = slice(max(w0, k0), min(w0 + d, k1))
                if cols.start >= cols.stop:
                    continue
                e = np.frexp(part[:, cols].max(axis=1))[1][:, None]  # max * 2^-e in [0.5, 1); 0 -> e = 0
                mant = _round_to(np.ldexp(part[:, cols], -e), torch.float16)
                part[:, cols] = np.ldexp(mant, e)
                used[:, cols] = np.ldexp(mant, e[np.arange(R) ^ 1] if swap_e else e)
        seen.append(torch.from_numpy(part).to(dtype) if fmt == "input" else torch.from_numpy(part.copy()))
        parts.append(used)
        with np.errstate(divide="ignore"):
            lses.append(np.where(st.l > 0, st.m + np.log2(st.l), -np.inf).astype(np.float32))
    M = np.max(lses, axis=0)
    acc, wsum = np.zeros((R, Lk), np.float32), np.zeros(R, np.float32)
    for part, lse in zip(parts, lses):
        wgt = _exp2_diff(lse, M)
        acc += wgt[:, None] * part
        wsum += wgt
    w = acc * (np.float32(1) / wsum)[:, None]
    return seen, lses, w, torch.from_numpy(w).to(dtype)


def _emulate_case(family, case, fmt, dtype, **defect):
    """emulate_partial_combine over every row of a case, in read_partials' shapes; also the fp32
    combined weights."""
    d, Lq, cr, Lk, kps = case
    _, _, s, P = _case(family, case, dtype)
    s2 = _base2(s, np.ones(s.shape, bool), d).reshape(B * H * Lq, Lk)
    if defect.get("drop_rows"):  # the last row of every chunk
        defect["drop_rows"] = np.arange(B * H * Lq) % Lq % cr == cr - 1
    seen, lses, w, out = emulate_partial_combine(s2, d, kps, fmt, dtype, **defect)
    raw = [x.reshape(B, H, Lq, Lk) for x in seen]
    return raw, [torch.from_numpy(l).reshape(B, H, Lq) for l in lses], out.reshape(B, H, Lq, Lk), w.reshape(P.shape)


# ----------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------


def test_partial_input_families_have_their_properties():
    """Per case, over the full key range (a shard's span is never larger): steep rows span at most
    40 log2 units, so that bf16 never meets its floor, and at least 20; every flat weight lies
    within e^(+-8) of 1 / Lk."""
    seen = {}
    for case, dtype in itertools.product(CASES + (STRIDED_CASE,), DTYPES):
        d, Lq, cr, Lk, kps = case
        assert Lq % cr == 0 and Lq % 2 == 0, case
        _, _, s, P = _case("flat", case, dtype)
        off = float(np.abs(np.log(P * Lk)).max())
        flat = float((s.max(-1) - s.min(-1)).max()) * LOG2E
        assert np.isfinite(s).all() and off < 8, (case, IDS[dtype], off)
        _, _, s, _ = _case("steep", case, dtype)
        span = (s.max(-1) - s.min(-1)) * LOG2E
        assert np.isfinite(s).all() and np.abs(s).max() < 1e3
        assert span.max() <= 40 and span.max() >= 20, (case, IDS[dtype], float(span.max()))
        seen[case, IDS[dtype]] = (round(float(span.max()), 1), round(flat, 1))
    print("partial cases (largest row span in log2 units: steep, flat):", seen)


def test_shard_weights_recombine_to_the_row():
    """The shard-local weights times the shards' shares of the row are the full-row weights."""
    case = CASES[0]
    _, _, s, P = _case("steep", case, torch.bfloat16)
    parts = [shard_weights(s, k0, k1) for k0, k1 in _shards(case[3], case[4])]
    lse = np.stack([x[2] for x in parts])
    w = np.exp2(lse - lse.max(0))
    w /= w.sum(0)
    assert np.abs(sum(wi[..., None] * x[0] for wi, x in zip(w, parts)) - P).max() <= 1e-12
    for P_loc, vis, _ in parts:
        assert (P_loc[~vis] == 0).all() and np.abs(P_loc.sum(-1) - 1).max() <= 1e-12


@pytest.mark.parametrize("fmt", PARTIAL_FORMATS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_partial_probe_reads_the_reference(dtype, fmt):
    """The probe's plumbing on the CPU: with the fp64 reference in the kernels' place (rounded
    once to the format, the chunk layout and {lse, e} as the kernels write them) every shard's
    partial, lse and the combined weights come back well inside their bounds."""
    for case in EMU_CASES:
        q, k, s, P = _case("flat", case, dtype)
        raw, lses, comb = read_partials(ref_partial, lambda o, l, f: ref_combine(o, l, f, dtype), case, q, k, fmt, dtype)
        worst = gate_partials(raw, lses, comb, case, s, P, fmt, dtype, f"probe {fmt}")
        # one rounding each (the 16-bit partial, the output), none on an fp32 partial or the lse
        assert worst[0] <= (0.01 if fmt == "fp32" else 0.5) and worst[1] <= 0.01 and worst[2] <= 0.5, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("family", FAMILIES)
def test_partial_emulation_stays_inside_the_bounds(family, dtype):
    """The kernels' steps, emulated, on the first and the last case: at most 0.75 of the raw
    partial's, the lse's and the combine's bound, per format."""
    for case in EMU_CASES:
        _, _, s, P = _case(family, case, dtype)
        for fmt in PARTIAL_FORMATS:
            raw, lses, comb, _ = _emulate_case(family, case, fmt, dtype)
            worst = gate_partials(raw, lses, comb, case, s, P, fmt, dtype, f"emulation {fmt}", limit=0.75)
            print(f"emulation partial {family} {IDS[dtype]} d={case[0]} {fmt}: raw / lse / combine",
                  [round(x, 3) for x in worst])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_readout_gate_rejects_partial_defects(dtype):
    """Two defects planted in the emulation (flat inputs, the first case): the readout gate
    rejects each; what the output gate (A + eps |ref| on P @ V, V ~ N(0, 1)) says to the same
    combined weights is printed."""
    case = CASES[0]
    d, Lq, cr, Lk, kps = case
    _, _, s, P = _case("flat", case, dtype)
    ones = np.ones(P.shape, bool)
    last = len(_shards(Lk, kps)) - 1
    P_loc, vis, _ = shard_weights(s, *_shards(Lk, kps)[last])

    def rejected(got, ref, vis_, **kw):
        leaked, bad, worst = readout_check(got, ref, vis_, dtype, **kw)
        return leaked > 0 or bad > 0 or worst > 1.0, (leaked, bad, round(worst, 2))

    for fmt in PARTIAL_FORMATS:  # the clean emulation passes both gates
        raw, _, comb, w = _emulate_case("flat", case, fmt, dtype)
        assert not rejected(comb, P, ones, extra=split_extra(P, d, kps, fmt, dtype))[0]
        assert _output_gate_accepts(w, P, dtype, 21)

    # 3. the last key of the last shard dropped in the last row of each chunk
    for fmt in PARTIAL_FORMATS:
        k_ulp, scaled = partial_bound(fmt)
        raw, _, comb, w = _emulate_case("flat", case, fmt, dtype, drop_rows=True)
        r, why = rejected(raw[last], P_loc, vis, k_ulp=k_ulp,
                          extra=split_extra(P_loc, d, kps, "scaled", dtype) if scaled else None)
        assert r, (fmt, why)
        rc, whyc = rejected(comb, P, ones, extra=split_extra(P, d, kps, fmt, dtype))
        assert rc, (fmt, whyc)
        print(f"dropped last key, last row of each chunk, {fmt}: raw readout", why, "combined readout", whyc,
              "output gate accepts:", _output_gate_accepts(w, P, dtype, 21))

    # 4. the combine applies row r's exponent to row r ^ 1 (scaled partials)
    raw, _, comb, w = _emulate_case("flat", case, "scaled", dtype, swap_e=True)
    r, why = rejected(comb, P, ones, extra=split_extra(P, d, kps, "scaled", dtype))
    assert r, why
    print("exponent of row r ^ 1 in the combine: readout", why, "output gate accepts:",
          _output_gate_accepts(w, P, dtype, 21))


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


def _partial_label(d, Lq, n_keys, strided=False):
    """What the library reports for a partial launch over a shard of n_keys keys."""
    name = "fa_fwd16_kernel" if d == 128 and n_keys % 64 == 0 else "fa_fwd_kernel"
    return f"{name}<partial{', strided' if strided else ''}> [grid {B * H * -(-Lq // 128)}]"


def _combine_label(d, Lq):
    return f"fa_combine_kernel [grid {-(-B * H * Lq * (d // 8) // 256)}]"


def _gpu_fns(ops, dtype):
    def partial(q, k_s, v_s, cr, fmt):
        return ops.attention_partial(q, k_s, v_s, chunk_rows=cr, partial_dtype=_pdtype(fmt, dtype))

    def combine(o_all, l_all, fmt):
        return ops.combine(o_all, l_all, B, H, dtype)

    return partial, combine


def _run(gpu, case, dtype, family, fmt):
    """read_partials on the device, the launch log asserted: per rotation every shard's partial
    kernel, then the combine."""
    from exploring_flash_attention_amd import ops
    d, Lq, cr, Lk, kps = case
    q, k, s, P = _case(family, case, dtype)
    with ops.launched_kernels() as kl:
        raw, lses, comb = read_partials(*_gpu_fns(ops, dtype), case, q, k, fmt, dtype, dev=gpu)
    want = [_partial_label(d, Lq, k1 - k0) for k0, k1 in _shards(Lk, kps)] + [_combine_label(d, Lq)]
    assert kl == want * _windows(Lk, d), kl
    return raw, lses, comb, s, P


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_readout_raw_partial(gpu, case, dtype, family):
    """Every shard's decoded partial against the shard-local weights, per format; columns of a
    probed window outside the shard read +-0."""
    d, _, _, Lk, kps = case
    worst = {}
    for fmt in PARTIAL_FORMATS:
        raw, _, _, s, _ = _run(gpu, case, dtype, family, fmt)
        k_ulp, scaled = partial_bound(fmt)
        worst[fmt] = 0.0
        for i, (k0, k1) in enumerate(_shards(Lk, kps)):
            P_loc, vis, _ = shard_weights(s, k0, k1)
            worst[fmt] = max(worst[fmt], readout_gate(
                raw[i], P_loc, vis, dtype, f"raw partial {fmt} shard {i}", quiet=True, k_ulp=k_ulp,
                extra=split_extra(P_loc, d, kps, "scaled", dtype) if scaled else None))
    print(f"readout op=partial dtype={IDS[dtype]} family={family} {CASE_IDS[CASES.index(case)]}: worst err/bound "
          "per partial format", {f: round(x, 3) for f, x in worst.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_partial_lse(gpu, case, dtype, family):
    """Every shard's lse against its fp64 base-2 lse, per format (the lse does not depend on V:
    one launch per shard; scaled: e an integer, asserted while decoding)."""
    from exploring_flash_attention_amd import ops
    d, Lq, cr, Lk, kps = case
    q, k, s, _ = _case(family, case, dtype)
    qd = q.to(gpu)
    v = selector(B, H, Lk, d, 0, dtype)
    worst = {}
    for fmt in PARTIAL_FORMATS:
        worst[fmt] = 0.0
        for k0, k1 in _shards(Lk, kps):
            with ops.launched_kernels() as kl:
                o_part, lse = _gpu_fns(ops, dtype)[0](qd, k[:, :, k0:k1].contiguous().to(gpu),
                                                     v[:, :, k0:k1].contiguous().to(gpu), cr, fmt)
            assert kl == [_partial_label(d, Lq, k1 - k0)], kl
            got = decode_partial(o_part, lse, fmt, dtype)[1].double().numpy()
            ref = shard_weights(s, k0, k1)[2]
            assert np.isfinite(got).all()
            worst[fmt] = max(worst[fmt], float((np.abs(got - ref) / lse_bound(ref, dtype)).max()))
    print(f"readout op=partial-lse dtype={IDS[dtype]} family={family} {CASE_IDS[CASES.index(case)]}: worst err/bound "
          "per partial format", {f: round(x, 3) for f, x in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_readout_combine(gpu, case, dtype, family):
    """ops.combine of all shards' partials against the full-row weights, per format."""
    d, _, _, _, kps = case
    worst = {}
    for fmt in PARTIAL_FORMATS:
        _, _, comb, _, P = _run(gpu, case, dtype, family, fmt)
        worst[fmt] = readout_gate(comb, P, np.ones(P.shape, bool), dtype, f"combine {fmt}", quiet=True,
                                  extra=split_extra(P, d, kps, fmt, dtype))
    print(f"readout op=combine dtype={IDS[dtype]} family={family} {CASE_IDS[CASES.index(case)]}: worst err/bound "
          "per partial format", {f: round(x, 3) for f, x in worst.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_readout_partial_strided_q(gpu, dtype, family):
    """The partial one destination chunk at a time from row-range views of q (fa_fwd_partial_ex,
    as the overlapped multi-GPU path computes it): bitwise the one-launch partial, lse and e
    included, and under the raw partial's gate."""
    from exploring_flash_attention_amd import ops
    case = STRIDED_CASE
    d, Lq, cr, Lk, kps = case
    nch = Lq // cr
    q, k, s, _ = _case(family, case, dtype)
    partial = _gpu_fns(ops, dtype)[0]

    def chunked(qd, k_s, v_s, cr_, fmt):
        scaled = fmt == "scaled"
        o = torch.empty(nch, B * H, cr, d, dtype=torch.float16 if scaled else _pdtype(fmt, dtype), device=gpu)
        lse = torch.empty((nch, B * H, cr, 2) if scaled else (nch, B * H, cr), dtype=torch.float32, device=gpu)
        for c in range(nch):
            rows = qd[:, :, c * cr:(c + 1) * cr]
            assert not rows.is_contiguous()
            ops.attention_partial(rows, k_s, v_s, partial_dtype=_pdtype(fmt, dtype), o_part=o[c][None], lse=lse[c][None])
        want_o, want_lse = partial(qd, k_s, v_s, cr, fmt)
        assert torch.equal(o.view(torch.int16), want_o.view(torch.int16)), fmt
        assert torch.equal(lse.view(torch.int32), want_lse.view(torch.int32)), fmt
        return o, lse

    worst = {}
    for fmt in PARTIAL_FORMATS:
        with ops.launched_kernels() as kl:
            raw, _, _ = read_partials(chunked, _gpu_fns(ops, dtype)[1], case, q, k, fmt, dtype, dev=gpu)
        want = []
        for k0, k1 in _shards(Lk, kps):
            want += [_partial_label(d, cr, k1 - k0, strided=True)] * nch + [_partial_label(d, Lq, k1 - k0)]
        assert kl == (want + [_combine_label(d, Lq)]) * _windows(Lk, d), kl
        k_ulp, scaled = partial_bound(fmt)
        worst[fmt] = 0.0
        for i, (k0, k1) in enumerate(_shards(Lk, kps)):
            P_loc, vis, _ = shard_weights(s, k0, k1)
            worst[fmt] = max(worst[fmt], readout_gate(
                raw[i], P_loc, vis, dtype, f"strided partial {fmt} shard {i}", quiet=True, k_ulp=k_ulp,
                extra=split_extra(P_loc, d, kps, "scaled", dtype) if scaled else None))
    print(f"readout op=partial-strided dtype={IDS[dtype]} family={family}: worst err/bound per partial format",
          {f: round(x, 3) for f, x in worst.items()})
