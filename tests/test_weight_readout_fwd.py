"""Softmax-weight readout of the full (non-causal) MHA forward, the chained persistent d = 128
kernels, the split-KV forward (attention_v2) and the variable-length forward (attention_varlen).

The probe, the fp64 reference weights, the gate K eps P + FLOOR, the input families and the NumPy
emulation are those of test_weight_readout.py (read its docstring first; the measured figures of
this file are in its table).  What this file adds:

Full forward.  (B, H, d, L) of CAUSAL_CASES with causal=False and H_kv == H: fa_fwd_kernel<final>
with and without a key tail, fa_fwd16_kernel<final> (d = 128, whole key tiles), and the strided
forms on [B, L, H, d] tensors.  Families flat and steep (tempt has no forbidden key here).

Chain.  fa_fwd16_chain_kernel<final> / <final, gqa> need at least one query tile per workgroup of
a grid of two workgroups per compute unit, so the cases are sized from the device (chain_cases):
every head, row and key is read, each head through another window, so a K or V tile carried over
a seam between two items of a workgroup's list shows in the columns of the head it came from.

Split-KV.  The one-shot fused kernels (store-first hand-off: d in {64, 128}, L in {512, 1000},
kv_tiles_per_block in {1, 4}, blocks_per_workgroup in {None, 1}; arrive-first: d = 128, two
blocks of 4096 keys), and fa_fwd16_chain_kernel<fused walk>, each under the three partial formats
with the bound K eps P + FLOOR + split_extra (derived from the format, see split_extra; fp32
partials: the bound as it stands).  The arrive-first case needs L = 8192: it probes the first
and the last window and the two on either side of the block edge at key 4096, 4 of 64 windows
(1 / 16 of the keys), every row.

Varlen.  test_varlen's ragged batch and its guard rows at max_seqlen 257 and 128 (truncation
inside a sequence); windows are relative to each sequence's start; V is NaN in every row of no
probed sequence (guard rows, rows cut by max_seqlen, the other sequences), and even and odd
sequences are probed in separate calls, so a neighbour's row that reaches P.V shows as NaN even
at zero weight; `out` is preset to a sentinel that the rows of no sequence must keep.  tempt:
the row after a sequence's end (the next sequence's first row, or a guard row, or the first row
cut by max_seqlen) is aligned with the sequence's last query row; causal: k[p + 1] = 1.5 q[p]
inside every sequence, that row included.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import test_varlen
from test_decode import DTYPES, IDS
from test_varlen import GUARD, SENTINEL, _cu_dev, varlen_ref
from test_weight_readout import (CAUSAL_CASES, FAMILIES, LOG2E, MANY_HEAD_STEEP, PARTIAL_FORMATS, SCALED_C, _gen,
                                 _scores, _softmax, _windows, chain_cases, fwd_inputs, fwd_weights, head_chunks,
                                 many_head_inputs, read_all, readout_gate, split_extra)

FULL_FAMILIES = FAMILIES[:2]
STRIDED_CASES = ((64, 200), (128, 200), (128, 384))  # one per strided kernel family, B = 2, H = 3
V2_SHAPES = [(d, L_) for d in (64, 128) for L_ in (512, 1000)]
V2_HEADS = (2, 8)  # (B, H): enough query tiles that the library's own grouping is not one block per workgroup
LONG_V2 = dict(L=8192, d=128, kvt=64, windows=(0, 31, 32, 63))  # two blocks of 4096 keys: the arrive-first hand-off
VARLEN_CASES = ([(d, causal, H, Hkv) for d in (64, 128) for causal in (False, True) for H, Hkv in ((4, 4), (4, 2))]
                + [(256, True, 4, 2)])
VARLEN_MSL = (257, 128)


def _pdtype(fmt, dtype):
    from exploring_flash_attention_amd import ops
    return {"fp32": torch.float32, "input": dtype, "scaled": ops.PARTIAL_FP16_SCALED}[fmt]


def gate_in_chunks(got, q, k, dtype, label, step=32, extra=None):
    """readout_gate of got [B, H, L, n] against the full forward's fp64 weights, computed in head
    chunks; extra: P -> the bound's extra term.  Prints and returns the worst err / bound."""
    worst = 0.0
    for h0, h1, qc, kc in head_chunks(q, k, step):
        P, vis, _ = fwd_weights(qc, kc, False)
        worst = max(worst, readout_gate(got[:, h0:h1], P, vis, dtype, f"{label} heads {h0}..{h1 - 1}", quiet=True,
                                        extra=None if extra is None else extra(P)))
    print(f"readout {label}: worst err/bound={worst:.3f}")
    return worst


# ----------------------------------------------------------------------------------------
# varlen: inputs, reference weights, the probe
# ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def varlen_inputs(family, d, H, Hkv, dtype, msl, causal):
    """Storage-rounded q [T, H, d], k [T, H_kv, d] of test_varlen's ragged batch with its guard
    rows; (q, k, cu, lens).  msl and causal matter to tempt only."""
    lens = test_varlen._lens(d)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(cu[-1]) + GUARD
    g = _gen("varlen", family, d, H, Hkv)
    q = (torch.randn(T, H, d, generator=g) * {"flat": 1.0, "steep": 3.0, "tempt": 2.0}[family]).to(dtype)
    k = torch.randn(T, Hkv, d, generator=g)
    if family == "tempt":
        G = H // Hkv
        for b, n in enumerate(lens):
            s, n = int(cu[b]), min(n, msl)
            if n == 0:
                continue
            if causal:  # key p + 1 is aligned with row p of the group's first head, the row after the end too
                k[s + 1:s + n + 1] = 1.5 * q[s:s + n, ::G].float()
            else:
                k[s + n] = 1.5 * q[s + n - 1, ::G].float()
    return q, k.to(dtype), cu, lens


def varlen_weights(q, k, cu, lens, msl, causal):
    """Per sequence (P, vis, s) [H, n, n], n = min(len, max_seqlen): the sequence's own rows, keys
    0..p of position p when causal, head h against K/V head h // G."""
    res = []
    for b, n in enumerate(lens):
        s0, n = int(cu[b]), min(n, msl)
        if n == 0:  # an empty sequence
            res.append((np.zeros((q.shape[1], 0, 0)), np.zeros((q.shape[1], 0, 0), bool), np.zeros((q.shape[1], 0, 0))))
            continue
        P, vis, s = fwd_weights(q[s0:s0 + n].transpose(0, 1)[None], k[s0:s0 + n].transpose(0, 1)[None], causal)
        res.append((P[0], vis[0], s[0]))
    return res


def varlen_selector(cu, lens, msl, T, Hkv, d, r, parity, dtype):
    """V [T, H_kv, d]: for the sequences b of this parity, K/V head hkv reads the window
    (b * H_kv + hkv + r) % windows of its own keys; NaN in every other row."""
    nw = _windows(min(max(lens), msl), d)
    v = torch.full((T, Hkv, d), float("nan"), dtype=dtype)
    for b, n in enumerate(lens):
        s, n = int(cu[b]), min(n, msl)
        if b % 2 != parity or n == 0:
            continue
        v[s:s + n] = 0
        for hkv in range(Hkv):
            j0 = (b * Hkv + hkv + r) % nw * d
            if j0 < n:
                c = torch.arange(min(d, n - j0))
                v[s + j0 + c, hkv, c] = 1
    return v


def read_varlen(call, q, cu, lens, msl, Hkv, d, dtype):
    """call(v, out) -> out [T, H, d] for every rotation and parity, `out` preset to the sentinel;
    per sequence the weights in key order [H, n, windows * d] (host, storage type).  Asserts that
    the rows of no sequence keep the sentinel in every call."""
    T, H = q.shape[:2]
    G = H // Hkv
    nw = _windows(min(max(lens), msl), d)
    owned = np.zeros(T, bool)
    for b, n in enumerate(lens):
        owned[int(cu[b]):int(cu[b]) + min(n, msl)] = True
    free = torch.from_numpy(~owned)
    got = [torch.full((H, min(n, msl), nw * d), float("nan"), dtype=dtype) for n in lens]
    for r, parity in itertools.product(range(nw), (0, 1)):
        out = call(varlen_selector(cu, lens, msl, T, Hkv, d, r, parity, dtype),
                   torch.full((T, H, d), SENTINEL, dtype=dtype))
        out = out.cpu()
        assert out.dtype == dtype and tuple(out.shape) == (T, H, d)
        assert (out[free].float() == SENTINEL).all(), f"a row of no sequence was written (r={r}, parity={parity})"
        for b, n in enumerate(lens):
            s, n = int(cu[b]), min(n, msl)
            if b % 2 != parity or n == 0:
                continue
            for hkv in range(Hkv):
                w, h0 = (b * Hkv + hkv + r) % nw, hkv * G
                got[b][h0:h0 + G, :, w * d:(w + 1) * d] = out[s:s + n, h0:h0 + G].transpose(0, 1)
    return got


def gate_varlen(got, ref, dtype, label):
    worst = 0.0
    for b, (x, (P, vis, _)) in enumerate(zip(got, ref)):
        if x.shape[1]:
            worst = max(worst, readout_gate(x, P, vis, dtype, f"{label} sequence {b}", quiet=True))
    return worst


# ----------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------


def test_varlen_weights_match_varlen_ref():
    """The per-sequence weights times a random fp64 V are varlen_ref, truncation included."""
    g = torch.Generator().manual_seed(9)
    lens = (5, 0, 37, 1, 20)
    cu = np.concatenate([[0], np.cumsum(lens)])
    T, H, Hkv, d = int(cu[-1]) + 3, 4, 2, 16
    q = torch.randn(T, H, d, generator=g, dtype=torch.float64)
    k, v = (torch.randn(T, Hkv, d, generator=g, dtype=torch.float64) for _ in range(2))
    for causal, msl in itertools.product((False, True), (64, 10)):
        want, _ = varlen_ref(q.numpy(), k.numpy(), v.numpy(), cu, msl, causal)
        for b, (P, vis, _) in enumerate(varlen_weights(q, k, cu, lens, msl, causal)):
            s, n = int(cu[b]), min(lens[b], msl)
            assert P.shape == (H, n, n) and (P[~vis] == 0).all()
            for h in range(H):
                assert n == 0 or np.abs(P[h] @ v.numpy()[s:s + n, h // 2] - want[s:s + n, h]).max() <= 1e-12, (b, h)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_varlen_probe_reads_the_reference(dtype):
    """The probe's plumbing on the CPU: with varlen_ref in the kernel's place (fp64, rounded once)
    every weight of every sequence comes back inside the bound, NaN rows and sentinel included."""
    d, causal, H, Hkv = 64, True, 4, 2
    for msl in VARLEN_MSL:
        q, k, cu, lens = varlen_inputs("flat", d, H, Hkv, dtype, msl, causal)

        def call(v, out):
            o, owned = varlen_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), cu, msl, causal)
            out[torch.from_numpy(owned)] = torch.from_numpy(o[owned]).to(dtype)
            return out

        got = read_varlen(call, q, cu, lens, msl, Hkv, d, dtype)
        assert gate_varlen(got, varlen_weights(q, k, cu, lens, msl, causal), dtype, "probe") <= 0.26  # one rounding


def test_varlen_input_families_have_their_properties():
    for (d, causal, H, Hkv), dtype, msl in itertools.product(VARLEN_CASES, DTYPES, VARLEN_MSL):
        G = H // Hkv
        h0 = np.arange(Hkv) * G
        for family in FAMILIES if msl == VARLEN_MSL[0] else FAMILIES[2:]:  # (flat, steep: the same q, k at any max_seqlen)
            q, k, cu, lens = varlen_inputs(family, d, H, Hkv, dtype, msl, causal)
            label = (family, d, causal, H, Hkv, IDS[dtype], msl)
            for b, (P, vis, s) in enumerate(varlen_weights(q, k, cu, lens, msl, causal)):
                n = P.shape[1]
                if n == 0:
                    continue
                hi, lo = np.where(vis, s, -np.inf), np.where(vis, s, np.inf)
                assert np.isfinite(s).all() and np.abs(s).max() < 1e3, label
                if family == "flat":
                    off = float(np.abs(np.log(np.where(vis, P * vis.sum(-1, keepdims=True), 1.0))).max())
                    assert off < 8, (label, b, off)
                elif family == "steep":
                    span = float((hi.max(-1) - lo.min(-1)).max()) * LOG2E
                    assert span <= 40, (label, b, span)
                else:  # the first key a row must not see carries that row's largest raw score
                    s0 = int(cu[b])
                    rows = np.arange(n) if causal else np.array([n - 1])
                    nxt = k[s0 + rows + 1].double().numpy()  # [rows, H_kv, d]
                    qq = q[s0 + rows][:, h0].double().numpy()
                    tempt = (qq * nxt).sum(-1).T / np.sqrt(d)  # [H_kv, rows]
                    assert (tempt > hi[h0][:, rows].max(-1)).all(), (label, b)


def test_long_split_case_has_the_family_properties():
    """The arrive-first case's inputs (one head of 8192 keys): built with their assertions."""
    for family in FULL_FAMILIES:
        _long_v2_case(family, torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _long_v2_case(family, dtype):
    """(q, k, P of the probed windows [1, 1, L, windows * d], the row maximum of P per window,
    same shape) of LONG_V2, the fp64 scores taken 1024 rows at a time."""
    L_, d, W = LONG_V2["L"], LONG_V2["d"], LONG_V2["windows"]
    g = _gen("v2-long", family)
    q = (torch.randn(1, 1, L_, d, generator=g) * {"flat": 1.0, "steep": MANY_HEAD_STEEP}[family]).to(dtype)
    k = torch.randn(1, 1, L_, d, generator=g).to(dtype)
    cols = np.concatenate([np.arange(w * d, (w + 1) * d) for w in W])
    P = np.empty((1, 1, L_, len(cols)))
    span = 0.0
    for r0 in range(0, L_, 1024):
        s = _scores(q[:, :, r0:r0 + 1024], k)
        span = max(span, float((s.max(-1) - s.min(-1)).max()) * LOG2E)
        P[:, :, r0:r0 + 1024] = _softmax(s, np.ones(s.shape, bool))[..., cols]
    assert span <= 40, (family, span)  # bf16 never meets its floor
    if family == "flat":
        assert np.abs(np.log(P * L_)).max() < 8
    mx = np.repeat(P.reshape(1, 1, L_, len(W), d).max(-1), d, axis=-1)
    P.setflags(write=False)
    return q, k, P, mx


# ----------------------------------------------------------------------------------------
# GPU: the full forward
# ----------------------------------------------------------------------------------------


def _v1_label(d, L_, nblk, strided=False):
    name = "fa_fwd16_kernel" if d == 128 and L_ % 64 == 0 else "fa_fwd_kernel"
    return f"{name}<final{', strided' if strided else ''}> [grid {nblk}]"


@pytest.mark.gpu
@pytest.mark.parametrize("family", FULL_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", CAUSAL_CASES, ids=lambda c: "B%d-H%d-d%d-L%d" % c)
def test_readout_full_forward(gpu, case, dtype, family):
    """fa_fwd_kernel<final> (key tail: every L but 384; none: d = 64 at L = 384) and
    fa_fwd16_kernel<final> (d = 128 at L = 384)."""
    from exploring_flash_attention_amd import ops
    B, H, d, L_ = case
    assert B * H >= _windows(L_, d)
    q, k = fwd_inputs(family, B, H, H, L_, d, dtype)
    qd, kd = q.to(gpu), k.to(gpu)
    with ops.launched_kernels() as kl:
        got = read_all(lambda v: ops.attention_v1(qd, kd, v.to(gpu)), B, H, H, L_, L_, d, dtype)
    assert kl == [_v1_label(d, L_, B * H * -(-L_ // 128))] * _windows(L_, d), kl
    gate_in_chunks(got, q, k, dtype, f"op=full dtype={IDS[dtype]} family={family} d={d} L={L_}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", FULL_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d,L_", STRIDED_CASES, ids=[f"d{d}-L{L_}" for d, L_ in STRIDED_CASES])
def test_readout_full_forward_strided(gpu, d, L_, dtype, family):
    """q, k, v and out as transposed views of [B, L, H, d] tensors, addressed in place."""
    from exploring_flash_attention_amd import ops
    B, H = 2, 3
    q, k = fwd_inputs(family, B, H, H, L_, d, dtype)
    view = lambda t: t.to(gpu).transpose(1, 2).contiguous().transpose(1, 2)
    qd, kd = view(q), view(k)
    assert not qd.is_contiguous()

    def call(v):
        out = torch.empty(B, L_, H, d, dtype=dtype, device=gpu).transpose(1, 2)
        return ops.attention_v1(qd, kd, view(v), out=out)

    with ops.launched_kernels() as kl:
        got = read_all(call, B, H, H, L_, L_, d, dtype)
    assert kl == [_v1_label(d, L_, B * H * -(-L_ // 128), strided=True)] * _windows(L_, d), kl
    gate_in_chunks(got, q, k, dtype, f"op=full-strided dtype={IDS[dtype]} family={family} d={d} L={L_}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", FULL_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("name", ("one-item", "uneven", "cross-head", "gqa"))
def test_readout_chain_forward(gpu, name, dtype, family):
    """fa_fwd16_chain_kernel<final> and <final, gqa>, every head, row and key (chain_cases)."""
    from exploring_flash_attention_amd import ops
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    grid = 2 * cus // 8 * 8
    H, Hkv, L_ = chain_cases(cus)[name]
    d, items = 128, H * (L_ // 128)
    assert items >= grid and (name == "one-item") == (items == grid)
    if name in ("uneven", "gqa"):
        assert grid < items < 2 * grid  # some workgroups run one item, some two
        assert name == "gqa" or items % 8 != 0  # ... and the XCD groups' item ranges are uneven
    q, k = many_head_inputs(family, H, Hkv, L_, d, dtype)
    qd, kd = q.to(gpu), k.to(gpu)
    with ops.launched_kernels() as kl:
        got = read_all(lambda v: ops.attention_v1(qd, kd, v.to(gpu)), 1, H, Hkv, L_, L_, d, dtype)
    label = "fa_fwd16_chain_kernel<final, gqa>" if Hkv < H else "fa_fwd16_chain_kernel<final>"
    assert kl == [f"{label} [grid {grid}]"] * (L_ // d), kl
    gate_in_chunks(got, q, k, dtype, f"op=chain-{name} dtype={IDS[dtype]} family={family} H={H}/{Hkv} L={L_}")


# ----------------------------------------------------------------------------------------
# GPU: split-KV
# ----------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("family", FULL_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d,L_", V2_SHAPES, ids=[f"d{d}-L{L_}" for d, L_ in V2_SHAPES])
def test_readout_split_kv(gpu, d, L_, dtype, family):
    """The one-shot fused kernels, store-first hand-off: key blocks of 64 and 256 keys, one block
    per workgroup and the library's grouping, L = 1000 with a key tail in the last split."""
    from exploring_flash_attention_amd import ops
    B, H = V2_HEADS
    q, k = fwd_inputs(family, B, H, H, L_, d, dtype)
    qd, kd = q.to(gpu), k.to(gpu)
    name = "fa_fwd16_kernel" if d == 128 and L_ % 64 == 0 else "fa_fwd_kernel"
    seen, worst = set(), dict.fromkeys(PARTIAL_FORMATS, 0.0)
    for kvt, bpw in itertools.product((1, 4), (1, None)):
        units, group, parts = ops.v2_split_plan(B, H, L_, d, kvt, dtype, blocks_per_workgroup=bpw)
        kps = group * kvt * 64
        assert units == -(-L_ // (kvt * 64)) and parts == -(-L_ // kps) and parts >= 2
        assert kps < 4096  # store-first
        if bpw == 1:
            assert group == 1
        if (kps, parts) in seen:  # the library's grouping is one block per workgroup here: the run above
            continue
        seen.add((kps, parts))
        for fmt in PARTIAL_FORMATS:
            with ops.launched_kernels() as kl:
                got = read_all(lambda v: ops.attention_v2(qd, kd, v.to(gpu), kvt, partial_dtype=_pdtype(fmt, dtype),
                                                          blocks_per_workgroup=bpw), B, H, H, L_, L_, d, dtype)
            want = f"{name}<fused split, in-kernel combine> [grid {B * H * -(-L_ // 128) * parts}]"
            assert kl == [want] * _windows(L_, d), kl
            worst[fmt] = max(worst[fmt], gate_in_chunks(
                got, q, k, dtype, f"op=v2 partials={fmt} dtype={IDS[dtype]} family={family} d={d} L={L_} "
                                  f"keys/split={kps} ({parts} partials)", step=4,
                extra=lambda P: split_extra(P, d, kps, fmt, dtype)))
    assert len(seen) >= 3
    print(f"readout op=v2 dtype={IDS[dtype]} family={family} d={d} L={L_}: worst err/bound per partial format",
          {f: round(x, 3) for f, x in worst.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("family", FULL_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_readout_split_kv_arrive_first(gpu, dtype, family):
    """fa_fwd16_kernel's arrive-first hand-off (key blocks of 4096 keys): L = 8192 in two blocks,
    one head; every row, the windows 0, 31, 32 (either side of the block edge) and 63 of 64."""
    from exploring_flash_attention_amd import ops
    L_, d, kvt, W = (LONG_V2[x] for x in ("L", "d", "kvt", "windows"))
    assert ops.v2_split_plan(1, 1, L_, d, kvt, dtype, blocks_per_workgroup=1) == (2, 1, 2) and kvt * 64 >= 4096
    q, k, P, mx = _long_v2_case(family, dtype)
    qd, kd = q.to(gpu), k.to(gpu)
    vis = np.ones(P.shape, bool)
    for fmt in PARTIAL_FORMATS:
        got = torch.empty(1, 1, L_, len(W) * d, dtype=dtype)
        with ops.launched_kernels() as kl:
            for i, w in enumerate(W):
                v = torch.zeros(1, 1, L_, d, dtype=dtype)
                c = torch.arange(d)
                v[0, 0, w * d + c, c] = 1
                got[..., i * d:(i + 1) * d] = ops.attention_v2(qd, kd, v.to(gpu), kvt, partial_dtype=_pdtype(fmt, dtype),
                                                               blocks_per_workgroup=1).cpu()
        assert kl == [f"fa_fwd16_kernel<fused split, in-kernel combine> [grid {L_ // 128 * 2}]"] * len(W), kl
        # every probed window lies inside one key block: its row maximum is split_extra's segment maximum
        extra = {"fp32": None, "input": split_extra(P, d, 4096, "input", dtype), "scaled": SCALED_C * 2.0 ** -24 * mx}[fmt]
        readout_gate(got, P, vis, dtype, f"op=v2-arrive-first partials={fmt} dtype={IDS[dtype]} family={family}",
                     extra=extra)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FULL_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("name", ("walk", "walk-uneven"))
def test_readout_split_kv_chained_walk(gpu, name, dtype, family):
    """fa_fwd16_chain_kernel<fused walk>: scaled fp16 partials, two blocks of 256 keys, four query
    tiles per head; the other two formats run the one-shot fused kernel on the same shape."""
    from exploring_flash_attention_amd import ops
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    grid = 2 * cus // 8 * 8
    H, _, L_ = chain_cases(cus)[name]
    d, kvt, kps = 128, 4, 256
    assert H * (L_ // 128) >= grid
    assert ops.v2_split_plan(1, H, L_, d, kvt, dtype, blocks_per_workgroup=1) == (2, 1, 2)
    q, k = many_head_inputs(family, H, H, L_, d, dtype)
    qd, kd = q.to(gpu), k.to(gpu)
    for fmt in PARTIAL_FORMATS:
        with ops.launched_kernels() as kl:
            got = read_all(lambda v: ops.attention_v2(qd, kd, v.to(gpu), kvt, partial_dtype=_pdtype(fmt, dtype),
                                                      blocks_per_workgroup=1), 1, H, H, L_, L_, d, dtype)
        want = (f"fa_fwd16_chain_kernel<fused walk> [grid {grid}]" if fmt == "scaled" else
                f"fa_fwd16_kernel<fused split, in-kernel combine> [grid {H * (L_ // 128) * 2}]")
        assert kl == [want] * (L_ // d), kl
        gate_in_chunks(got, q, k, dtype, f"op=v2-{name} partials={fmt} dtype={IDS[dtype]} family={family} H={H}",
                       extra=lambda P: split_extra(P, d, kps, fmt, dtype))


# ----------------------------------------------------------------------------------------
# GPU: varlen
# ----------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d,causal,H,Hkv", VARLEN_CASES,
                         ids=[f"d{d}-{'causal' if c else 'full'}-H{H}-Hkv{Hkv}" for d, c, H, Hkv in VARLEN_CASES])
def test_readout_varlen(gpu, d, causal, H, Hkv, dtype, family):
    """The ragged batch at max_seqlen 257 (three query tiles) and 128 (sequences cut)."""
    from exploring_flash_attention_amd import ops
    worst = 0.0
    for msl in VARLEN_MSL:
        q, k, cu, lens = varlen_inputs(family, d, H, Hkv, dtype, msl, causal)
        qd, kd, cud = q.to(gpu), k.to(gpu), _cu_dev(cu, gpu)
        with ops.launched_kernels() as kl:
            got = read_varlen(lambda v, out: ops.attention_varlen(qd, kd, v.to(gpu), cud, msl, causal=causal,
                                                                  out=out.to(gpu)), q, cu, lens, msl, Hkv, d, dtype)
        label = "fa_fwd_kernel<final, varlen" + (", causal" if causal else "") + (", gqa" if Hkv < H else "") + ">"
        assert kl == [f"{label} [grid {len(lens) * H * -(-msl // 128)}]"] * (2 * _windows(msl, d)), kl
        worst = max(worst, gate_varlen(got, varlen_weights(q, k, cu, lens, msl, causal), dtype,
                                       f"varlen max_seqlen={msl}"))
    print(f"readout op=varlen dtype={IDS[dtype]} family={family} d={d} causal={causal} H={H}/{Hkv}: "
          f"worst err/bound={worst:.3f}")
