"""KV-cache decode attention: ops.attention_decode / fa_fwd_decode / fa_fwd_decode_plan.

q [B, H, Lq, d] (Lq small) against k, v [B, H_kv, Lk, d] with per-sequence key lengths and a
bottom-right aligned causal mask; the G * Lq query rows of a K/V head are one work item's query
tile and the keys are split over the chip (csrc/fa_decode.hip).

CPU: the fp64 reference of this file against torch SDPA with an explicit mask, exports, argument
checks, Python refusals, planner properties at cus = 256 and an address replay of the kernel's
work items.  GPU: parity with the fp64 reference under the project's gate
|out - ref| <= A + eps * |ref| plus the mean relative error -- bf16 (6e-3, 1e-2, 2^-8), fp16
(2e-3, 3e-3, 2^-11), the values of test_causal.py / test_gqa.py, unchanged because the partials
are fp32 -- and the bitwise properties (cache garbage, clamp, strides, isolation, reuse).
"""
import ctypes
import functools
import itertools
import subprocess

import numpy as np
import pytest
import torch

import exploring_flash_attention_amd._lib as L

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x10000)

GATE = {torch.bfloat16: (6e-3, 1e-2, 2.0 ** -8), torch.float16: (2e-3, 3e-3, 2.0 ** -11)}
DTYPES = (torch.bfloat16, torch.float16)
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}
HEADS = ((4, 2), (8, 1), (4, 4))
TILE = 64


def decode_ref(q, k, v, seqlens=None, causal=True, scale=None):
    """fp64 reference: q [B, H, Lq, d], k / v [B, H_kv, Lk, d] (NumPy).  Query head h reads K/V
    head h // G; batch b has len_b = clamp(seqlens[b], 0, Lk) keys; causal: row position i sees
    keys j <= len_b - Lq + i; a row without a visible key is zero."""
    B, H, Lq, d = q.shape
    Hkv, Lk = k.shape[1], k.shape[2]
    G = H // Hkv
    scale = 1.0 / np.sqrt(d) if scale is None else scale
    out = np.zeros((B, H, Lq, v.shape[3]), np.float64)
    for b in range(B):
        n = Lk if seqlens is None else min(max(int(seqlens[b]), 0), Lk)
        for h in range(H):
            for i in range(Lq):
                vis = min(n, n - Lq + i + 1) if causal else n
                if vis <= 0:
                    continue
                s = (k[b, h // G, :vis].astype(np.float64) @ q[b, h, i].astype(np.float64)) * scale
                p = np.exp(s - s.max())
                out[b, h, i] = (p / p.sum()) @ v[b, h // G, :vis].astype(np.float64)
    return out


# ----------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------


def test_decode_reference_matches_torch_sdpa():
    B, H, Hkv, Lq, Lk, d = 3, 6, 2, 4, 23, 16
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, H, Lq, d, generator=g, dtype=torch.float64)
    k, v = (torch.randn(B, Hkv, Lk, d, generator=g, dtype=torch.float64) for _ in range(2))
    ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    for seqlens, causal in itertools.product((None, [23, 9, 2], [0, 3, 40]), (False, True)):
        mask = torch.zeros(B, 1, Lq, Lk, dtype=torch.bool)
        for b in range(B):
            n = Lk if seqlens is None else min(max(seqlens[b], 0), Lk)
            for i in range(Lq):
                vis = min(n, n - Lq + i + 1) if causal else n
                mask[b, 0, i, :max(vis, 0)] = True
        got = decode_ref(q.numpy(), k.numpy(), v.numpy(), seqlens, causal)
        want = torch.nn.functional.scaled_dot_product_attention(q, ke, ve, attn_mask=mask).numpy()
        has = mask.any(dim=-1).expand(B, H, Lq).numpy()
        assert np.abs(got[has] - want[has]).max() <= 1e-12, (seqlens, causal)
        assert (got[~has] == 0).all(), (seqlens, causal)
        if seqlens == [23, 9, 2] and causal:  # len 2 < Lq 4: rows 0, 1 see nothing, rows 2, 3 one and two keys
            assert not has[2, :, :2].any() and has[2, :, 2:].all()
        if seqlens == [0, 3, 40]:
            assert not has[0].any() and (got[0] == 0).all()


def test_decode_entries_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in ("fa_fwd_decode", "fa_fwd_decode_plan"):
        assert name in names and name in L.SIGNATURES
    assert L.lib().fa_version() == 0x000400


def test_decode_entry_argument_checks():
    lib = L.lib()
    BF = L.FA_DTYPE_BF16
    BIG = 1 << 30  # "enough" workspace bytes: nothing is launched before a check fails

    def err():
        return lib.fa_last_error()

    def call(q=FAKE, k=FAKE, v=FAKE, o=FAKE, sl=NULL, B=1, H=4, Hkv=2, Lq=1, Lk=640, d=128, st=None, scale=0.1,
             flags=0, ns=2, ws=FAKE, wsb=BIG, dt=BF):
        return lib.fa_fwd_decode(q, k, v, o, sl, B, H, Hkv, Lq, Lk, d, st, scale, flags, ns, ws, wsb, dt, NULL)

    INV, UNS = L.FA_ERR_INVALID_ARG, L.FA_ERR_UNSUPPORTED
    # null and misaligned pointers
    for name in ("q", "k", "v", "o"):
        assert call(**{name: NULL}) == INV and b"null" in err()
        assert call(**{name: ctypes.c_void_p(0x10002)}) == INV and b"aligned" in err()
    assert call(sl=ctypes.c_void_p(0x10002)) == INV and b"seqlens_k" in err()
    # sizes
    for name in ("B", "H", "Lq", "Lk", "d"):
        assert call(**{name: 0}) == INV and b"positive" in err(), name
    # H_kv: positive, at most H, a divisor of H
    for hkv in (0, -1, 8, 3):
        assert call(Hkv=hkv) == INV and b"H_kv" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(scale=bad) == INV and b"softmax_scale" in err()
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == INV and b"flags" in err()
    assert call(ns=-1) == INV and b"num_splits" in err()
    # workspace: two splits need one
    assert call(ws=NULL) == INV and b"workspace" in err()
    assert call(wsb=16) == INV and b"workspace" in err()
    assert call(ws=ctypes.c_void_p(0x10004)) == INV and b"workspace" in err()
    # K/V strides: positive multiples of 8, rows at least d apart
    for bad in ((0, 128, 128), (81920, 4, 128), (81920, 81920, 64)):
        assert call(st=(ctypes.c_int64 * 3)(*bad)) == INV and b"stride" in err(), bad
    # no kernel: head dims, packed rows, fp64
    for d in (32, 96, 256):
        assert call(d=d) == UNS and b"decode" in err() and str(d).encode() in err()
    assert call(H=8, Hkv=1, Lq=9) == UNS and b"64" in err() and b"Lq" in err()  # 8 * 9 = 72 rows
    assert call(H=4, Hkv=4, Lq=65) == UNS and b"Lq" in err()
    assert call(dt=L.FA_DTYPE_FP64) == UNS and b"FP64" in err()
    # the planner shares the shape checks
    s, kps, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    plan = lib.fa_fwd_decode_plan
    assert plan(1, 4, 3, 1, 640, 128, 0, 256, BF, s, kps, nb) == INV and b"H_kv" in err()
    assert plan(1, 4, 2, 1, 640, 96, 0, 256, BF, s, kps, nb) == UNS and b"d=96" in err()
    assert plan(1, 4, 2, 1, 640, 128, -2, 256, BF, s, kps, nb) == INV and b"num_splits" in err()
    assert plan(1, 4, 2, 1, 640, 128, 0, -1, BF, s, kps, nb) == INV and b"cus" in err()
    assert plan(1, 4, 2, 1, 640, 128, 0, 256, BF, None, None, None) == L.FA_OK


def test_decode_python_refusals(monkeypatch):
    import exploring_flash_attention_amd as fa
    from exploring_flash_attention_amd import ops
    assert fa.attention_decode is ops.attention_decode and "attention_decode" in fa.__all__
    assert "attention_decode" in fa.__doc__
    bf = torch.bfloat16
    q = torch.zeros(2, 4, 1, 128, dtype=bf)
    kv = torch.zeros(2, 2, 64, 128, dtype=bf)
    with pytest.raises(ValueError, match="no CPU fallback"):  # host tensors: refused as everywhere
        ops.attention_decode(q, kv, kv)
    # the checks behind the device check, on host tensors (nothing is launched before they raise)
    monkeypatch.setattr(ops, "_check_tensor", lambda *a, **k: None)
    k3 = torch.zeros(2, 3, 64, 128, dtype=bf)
    with pytest.raises(ValueError, match="multiple"):
        ops.attention_decode(q, k3, k3)
    with pytest.raises(NotImplementedError, match="attention_v1"):  # R = 65
        ops.attention_decode(torch.zeros(2, 2, 65, 128, dtype=bf), kv, kv)
    with pytest.raises(NotImplementedError, match="attention_v1"):  # R = 2 * 33
        ops.attention_decode(torch.zeros(2, 4, 33, 128, dtype=bf), kv, kv)
    with pytest.raises(NotImplementedError, match="d=256"):
        ops.attention_decode(torch.zeros(2, 4, 1, 256, dtype=bf), torch.zeros(2, 2, 64, 256, dtype=bf),
                             torch.zeros(2, 2, 64, 256, dtype=bf))
    with pytest.raises(NotImplementedError, match="float64"):
        ops.attention_decode(q.double(), kv.double(), kv.double())
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                torch.zeros(2, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="seqlens_k"):
            ops.attention_decode(q, kv, kv, seqlens_k=bad)
    with pytest.raises(ValueError, match="same shape"):
        ops.attention_decode(q, kv, k3)
    # the other operators keep their refusals (Lq != Lk, H_kv < H)
    with pytest.raises(ValueError, match="same shape"):
        ops.attention_v1(q, kv, kv)
    for call in (lambda: ops.attention_v2(q, kv, kv), lambda: ops.attention_partial(q, kv, kv),
                 lambda: ops.attention_tiled_d(q, kv, kv)):
        with pytest.raises(ValueError, match="attention_v1 only"):
            call()


PLAN_GRID = [(B, Hkv, Lq, Lk, d, ns)
             for B in (1, 2, 16, 64) for Hkv in (1, 2, 8) for Lq in (1, 4) for Lk in (1, 63, 64, 65, 200, 1041, 8192, 100000)
             for d in (64, 128) for ns in (None, 1, 2, 5, 7, 4096)]


def test_decode_planner_properties():
    from exploring_flash_attention_amd import ops
    for B, Hkv, Lq, Lk, d, ns in PLAN_GRID:
        H = 4 * Hkv
        R = 4 * Lq
        splits, kps, nbytes = ops.decode_plan(B, H, Hkv, Lq, Lk, d, ns, cus=256)
        tiles = -(-Lk // TILE)
        assert kps % TILE == 0 and kps > 0
        assert splits * kps >= Lk and (splits - 1) * kps < Lk, (B, Hkv, Lq, Lk, d, ns, splits, kps)
        assert 1 <= splits <= tiles
        if ns is not None:
            assert splits <= min(ns, tiles)
            if min(ns, tiles) <= 2 or tiles % min(ns, tiles) == 0:
                assert splits == min(ns, tiles)
        else:
            if B * Hkv >= 256:
                assert splits == 1
            if splits > 1:  # as few as fill the chip: one split fewer would not
                assert (splits - 1) * B * Hkv < 256
        # the workspace covers every item's partial O and lse (no counters: a second kernel combines)
        items = B * Hkv * splits
        assert nbytes == 0 if splits == 1 else nbytes >= items * R * d * 4 + items * R * 4
        # fp16 plans alike
        assert ops.decode_plan(B, H, Hkv, Lq, Lk, d, ns, dtype=torch.float16, cus=256) == (splits, kps, nbytes)
    assert ops.decode_plan(64, 32, 8, 1, 8192, 128, cus=256)[0] == 1
    s, kps, _ = ops.decode_plan(1, 32, 8, 1, 8192, 128, cus=256)
    assert s * 1 * 8 >= 256 and s > 1
    # fewer compute units, fewer splits
    assert ops.decode_plan(1, 32, 8, 1, 8192, 128, cus=64)[0] < s


# ---- address replay of csrc/fa_decode.hip: item (b, hkv, split) = ((b * Hkv + hkv) * splits + s)


def decode_replay(B, H, Hkv, Lq, Lk, d, ns, kv_shape, kv_view, seqlens=None, kv_base=None):
    """Walk every work item of the plan as the kernel does and check every byte range it touches.
    kv_shape: the cache allocation; kv_view: maps it to the [B, Hkv, Lk, d] view the call gets.
    kv_base(b, hkv, H, G, strides): element offset of the item's K/V head (the kernel's rule
    unless a mutation is passed).  Returns the number of K/V tiles walked."""
    from exploring_flash_attention_amd import ops
    G = H // Hkv
    R = G * Lq
    splits, kps, nbytes = ops.decode_plan(B, H, Hkv, Lq, Lk, d, ns, cus=256)
    alloc = torch.empty(kv_shape, dtype=torch.bfloat16, device="meta")
    view = kv_view(alloc)
    assert tuple(view.shape) == (B, Hkv, Lk, d) and view.stride(3) == 1
    st = view.stride()[:3]
    alloc_bytes = alloc.numel() * 2
    off0 = view.storage_offset()
    if kv_base is None:
        def kv_base(b, hkv, H, G, st):
            return b * st[0] + hkv * st[1]
    q_bytes = B * H * Lq * d * 2
    o_part_bytes = (B * Hkv * splits * R * d * 4 + 255) // 256 * 256 if splits > 1 else 0
    slots, tiles = [], 0
    for b, hkv, s in itertools.product(range(B), range(Hkv), range(splits)):
        item = (b * Hkv + hkv) * splits + s
        n = Lk if seqlens is None else min(max(seqlens[b], 0), Lk)
        # Q / O: the group's rows are the block of query heads hkv * G .. hkv * G + G - 1
        blk = (b * Hkv + hkv) * R * d * 2
        assert blk == ((b * H + hkv * G) * Lq) * d * 2 and blk + R * d * 2 <= q_bytes
        if splits > 1:
            slots.append((item * R * d * 4, item * R * d * 4 + R * d * 4))
            slots.append((o_part_bytes + item * R * 4, o_part_bytes + item * R * 4 + R * 4))
        kv_begin, kv_end = s * kps, min(s * kps + kps, n)
        assert kv_begin < Lk  # no structurally empty split
        if kv_begin >= n:
            continue
        head = kv_base(b, hkv, H, G, st)
        for t in range(-(-(kv_end - kv_begin) // TILE)):
            row0 = kv_begin + t * TILE
            nv = min(TILE, kv_end - row0)
            lo = (off0 + head + row0 * st[2]) * 2
            hi = lo + (nv - 1) * st[2] * 2 + d * 2
            assert 0 <= lo and hi <= alloc_bytes, ("K/V tile outside the allocation", b, hkv, s, t)
            # ... and it is the tile of this batch and K/V head
            want = (off0 + b * st[0] + hkv * st[1] + row0 * st[2]) * 2
            assert lo == want, ("K/V tile of another head", b, hkv, s, t)
            tiles += 1
    slots.sort()
    for (a0, a1), (b0, b1) in zip(slots, slots[1:]):
        assert a1 <= b0, "partial slots overlap"
    if slots:
        assert slots[0][0] >= 0 and slots[-1][1] <= nbytes
    return tiles


REPLAY = ((2, 4, 2, 3, 1041, 128, None), (2, 8, 1, 8, 200, 64, 5), (3, 4, 4, 1, 65, 128, 2), (1, 32, 8, 1, 8192, 128, None))


@pytest.mark.parametrize("case", REPLAY, ids=lambda c: "B%d-H%d-Hkv%d-Lq%d-Lk%d-d%d-ns%s" % c)
def test_decode_address_replay(case):
    B, H, Hkv, Lq, Lk, d, ns = case
    n = decode_replay(B, H, Hkv, Lq, Lk, d, ns, (B, Hkv, Lk, d), lambda a: a)
    assert n == B * Hkv * -(-Lk // TILE)
    # a [B, Lmax, H_kv, d] cache viewed as [B, H_kv, Lk, d]
    Lmax = Lk + 37
    assert decode_replay(B, H, Hkv, Lq, Lk, d, ns, (B, Lmax, Hkv, d), lambda a: a.transpose(1, 2)[:, :, :Lk]) == n
    # per-sequence lengths only shorten the walk
    assert decode_replay(B, H, Hkv, Lq, Lk, d, ns, (B, Hkv, Lk, d), lambda a: a, seqlens=[Lk] + [min(37, Lk)] * (B - 1)) <= n


def test_decode_replay_catches_wrong_kv_bases():
    B, H, Hkv, Lq, Lk, d = 2, 4, 2, 3, 200, 128
    for shape, view in (((B, Hkv, Lk, d), lambda a: a), ((B, Lk, Hkv, d), lambda a: a.transpose(1, 2))):
        decode_replay(B, H, Hkv, Lq, Lk, d, 2, shape, view)
        with pytest.raises(AssertionError, match="K/V tile"):  # the base of the query head b * H + h
            decode_replay(B, H, Hkv, Lq, Lk, d, 2, shape, view,
                          kv_base=lambda b, hkv, H, G, st: (b * H + hkv * G) * st[1])
        with pytest.raises(AssertionError, match="K/V tile"):  # the batch term dropped
            decode_replay(B, H, Hkv, Lq, Lk, d, 2, shape, view, kv_base=lambda b, hkv, H, G, st: hkv * st[1])


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _inputs(B, H, Hkv, Lq, Lk, d, dtype, seed=0):
    """Seeded storage-rounded host inputs, computed once and shared; nobody writes to them."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Lq, d, generator=g).to(dtype)
    k, v = (torch.randn(B, Hkv, Lk, d, generator=g).to(dtype) for _ in range(2))
    return q, k, v


@functools.lru_cache(maxsize=None)
def _ref(B, H, Hkv, Lq, Lk, d, dtype, causal, seqlens=None, seed=0):
    q, k, v = _inputs(B, H, Hkv, Lq, Lk, d, dtype, seed)
    ref = decode_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), seqlens, causal)
    ref.setflags(write=False)
    return ref


def _gate(out, ref, dtype, label="", quiet=False):
    out = out.float().cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert np.isfinite(out).all(), label
    A, mean_rel_tol, eps = GATE[dtype]
    err = np.abs(out - ref)
    bound = A + eps * np.abs(ref)
    worst = float((err / bound).max()) if err.size else 0.0
    big = np.abs(ref) > 1e-3
    mean_rel = float((err[big] / np.abs(ref[big])).mean()) if big.any() else 0.0
    if not quiet:
        print(f"{label}: max_abs={err.max() if err.size else 0.0:.3e} worst err/bound={worst:.3f} mean_rel={mean_rel:.3e}")
    assert worst <= 1.0, (label, worst, float(err.max()))
    assert mean_rel <= mean_rel_tol, (label, mean_rel)
    return worst


def _sl(seqlens, gpu):
    return None if seqlens is None else torch.tensor(seqlens, dtype=torch.int32, device=gpu)


def _bits(t):
    return t.view(torch.int16).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("Lk", (1, 63, 64, 65, 200, 1041))
@pytest.mark.parametrize("d", (64, 128))
def test_decode_matches_fp64_reference(gpu, d, Lk, dtype, causal):
    from exploring_flash_attention_amd import ops
    worst = 0.0
    for (H, Hkv), Lq in itertools.product(HEADS, (1, 3, 8)):
        q, k, v = _inputs(2, H, Hkv, Lq, Lk, d, dtype)
        qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
        for seqlens in (None, (Lk, min(37, Lk))):
            ref = _ref(2, H, Hkv, Lq, Lk, d, dtype, causal, seqlens)
            for ns in (None, 1, 2, 5):
                with ops.launched_kernels() as kl:
                    o = ops.attention_decode(qd, kd, vd, seqlens_k=_sl(seqlens, gpu), causal=causal, num_splits=ns)
                assert o.dtype == dtype and tuple(o.shape) == (2, H, Lq, d)
                splits = ops.decode_plan(2, H, Hkv, Lq, Lk, d, ns, dtype)[0]
                assert len(kl) == 1 and kl[0].startswith("fa_decode_kernel<"), kl
                assert f"[grid {2 * Hkv * splits}]" in kl[0].split(" + ")[0], (kl, splits)
                assert ("fa_decode_combine_kernel" in kl[0]) == (splits > 1), kl
                worst = max(worst, _gate(o, ref, dtype, f"decode H{H}/{Hkv} Lq{Lq} Lk{Lk} d{d} {IDS[dtype]} causal={causal} "
                                                     f"seqlens={seqlens} ns={ns}", quiet=True))
    print(f"worst err/bound over heads, Lq, seqlens, splits: {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_decode_empty_and_short_sequences(gpu, d, dtype):
    from exploring_flash_attention_amd import ops
    H, Hkv, Lk = 4, 2, 200
    for ns, causal in itertools.product((None, 1, 3), (False, True)):
        # an empty sequence: exactly zero
        q, k, v = _inputs(2, H, Hkv, 3, Lk, d, dtype)
        o = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu), seqlens_k=_sl((0, Lk), gpu), causal=causal, num_splits=ns)
        assert (_bits(o[0]) == 0).all(), (ns, causal)
        ref = _ref(2, H, Hkv, 3, Lk, d, dtype, causal, (0, Lk))
        _gate(o[1:], ref[1:], dtype, f"len (0, {Lk}) ns={ns} causal={causal}")
    for ns in (None, 1, 3):
        # len 2 < Lq 3, causal: row 0 sees nothing, rows 1 and 2 see one and two keys
        o = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu), seqlens_k=_sl((2, Lk), gpu), causal=True, num_splits=ns)
        assert (_bits(o[0, :, 0]) == 0).all(), ns
        _gate(o, _ref(2, H, Hkv, 3, Lk, d, dtype, True, (2, Lk)), dtype, f"len (2, {Lk}) ns={ns}")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_decode_empty_splits(gpu, dtype, causal):
    from exploring_flash_attention_amd import ops
    for d, Lq in ((64, 1), (128, 3)):
        q, k, v = _inputs(2, 4, 2, Lq, 1041, d, dtype)
        assert ops.decode_plan(2, 4, 2, Lq, 1041, d, 5, dtype)[0] == 5
        o = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu), seqlens_k=_sl((37, 1041), gpu), causal=causal, num_splits=5)
        _gate(o, _ref(2, 4, 2, Lq, 1041, d, dtype, causal, (37, 1041)), dtype, f"empty splits d{d} Lq{Lq} causal={causal}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_decode_ignores_cache_garbage(gpu, d, dtype):
    from exploring_flash_attention_amd import ops
    H, Hkv, Lq, Lk = 4, 2, 3, 200
    lens = (150, 37)
    huge = 3e38 if dtype == torch.bfloat16 else 6e4
    q, k, v = _inputs(2, H, Hkv, Lq, Lk, d, dtype)
    qd = q.to(gpu)
    for ns, causal in itertools.product((None, 1, 3), (False, True)):
        outs = []
        for fill in (0.0, float("nan"), huge):
            kg, vg = k.clone(), v.clone()
            for b, n in enumerate(lens):
                kg[b, :, n:] = fill
                vg[b, :, n:] = fill
            outs.append(ops.attention_decode(qd, kg.to(gpu), vg.to(gpu), seqlens_k=_sl(lens, gpu), causal=causal, num_splits=ns))
        _gate(outs[0], _ref(2, H, Hkv, Lq, Lk, d, dtype, causal, lens), dtype, f"garbage ns={ns} causal={causal}", quiet=True)
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), ("NaN past len", ns, causal)
        assert torch.equal(_bits(outs[0]), _bits(outs[2])), ("huge past len", ns, causal)
    # the keys a causal row may not see: row position i does not see the last Lq - 1 - i keys
    for ns, lens in itertools.product((None, 1, 3), (None, (150, 37))):
        clean = ops.attention_decode(qd, k.to(gpu), v.to(gpu), seqlens_k=_sl(lens, gpu), causal=True, num_splits=ns)
        for i in range(Lq - 1):
            vg = v.clone()
            for b in range(2):
                n = Lk if lens is None else lens[b]
                vg[b, :, n - (Lq - 1 - i):n] = float("nan")
            o = ops.attention_decode(qd, k.to(gpu), vg.to(gpu), seqlens_k=_sl(lens, gpu), causal=True, num_splits=ns)
            assert torch.equal(_bits(o[:, :, :i + 1]), _bits(clean[:, :, :i + 1])), ("NaN V behind the mask", ns, lens, i)
            assert torch.isnan(o[:, :, Lq - 1].float()).all()  # the last row does see them


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_decode_clamps_lengths_to_lk(gpu, dtype):
    from exploring_flash_attention_amd import ops
    H, Hkv, Lq, d = 4, 2, 3, 128
    q, k, v = _inputs(2, H, Hkv, Lq, 264, d, dtype)
    kd, vd = k.clone(), v.clone()
    kd[:, :, 200:] = float("nan")
    vd[:, :, 200:] = float("nan")
    kd, vd = kd.to(gpu)[:, :, :200], vd.to(gpu)[:, :, :200]  # rows 200..263 of the allocation hold NaN
    assert not kd.is_contiguous()
    for ns, causal in itertools.product((None, 1, 2), (False, True)):
        a = ops.attention_decode(q.to(gpu), kd, vd, seqlens_k=_sl((300, 200), gpu), causal=causal, num_splits=ns)
        b = ops.attention_decode(q.to(gpu), kd, vd, causal=causal, num_splits=ns)
        assert torch.isfinite(a.float()).all()
        assert torch.equal(_bits(a), _bits(b)), (ns, causal)
    ref = decode_ref(q.double().numpy(), k[:, :, :200].double().numpy(), v[:, :, :200].double().numpy(), None, True)
    _gate(ops.attention_decode(q.to(gpu), kd, vd, seqlens_k=_sl((300, 200), gpu)), ref, dtype, "clamped lengths")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_decode_reads_a_strided_cache_in_place(gpu, d, dtype):
    from exploring_flash_attention_amd import ops
    B, H, Hkv, Lq, Lk, Lmax = 2, 4, 2, 3, 200, 256
    q, k, v = _inputs(B, H, Hkv, Lq, Lk, d, dtype)
    kc, vc = (torch.full((B, Lmax, Hkv, d), float("nan"), dtype=dtype, device=gpu) for _ in range(2))
    kc[:, :Lk] = k.to(gpu).transpose(1, 2)
    vc[:, :Lk] = v.to(gpu).transpose(1, 2)
    kv_, vv_ = kc.transpose(1, 2)[:, :, :Lk], vc.transpose(1, 2)[:, :, :Lk]
    assert not kv_.is_contiguous() and kv_.stride() == (Lmax * Hkv * d, d, Hkv * d, 1)
    for ns, causal, lens in itertools.product((None, 2), (False, True), (None, (200, 37))):
        want = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu), seqlens_k=_sl(lens, gpu), causal=causal, num_splits=ns)
        with ops.launched_kernels() as kl:
            got = ops.attention_decode(q.to(gpu), kv_, vv_, seqlens_k=_sl(lens, gpu), causal=causal, num_splits=ns)
        assert len(kl) == 1 and kl[0].count("fa_decode_kernel<") == 1 and "fa_fwd" not in kl[0], kl
        assert torch.equal(_bits(got), _bits(want)), (ns, causal, lens)
    _gate(got, _ref(B, H, Hkv, Lq, Lk, d, dtype, True, (200, 37)), dtype, "strided cache")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_decode_group_isolation(gpu, causal):
    from exploring_flash_attention_amd import ops
    q, k, v = _inputs(2, 4, 2, 3, 200, 128, torch.bfloat16)
    base = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu), causal=causal, num_splits=2)
    k2, v2 = k.clone(), v.clone()
    k2[:, 1] *= 50
    v2[:, 1] *= 50
    o = ops.attention_decode(q.to(gpu), k2.to(gpu), v2.to(gpu), causal=causal, num_splits=2)
    assert torch.equal(_bits(o[:, :2]), _bits(base[:, :2]))  # query heads 0, 1 read K/V head 0
    assert not torch.equal(_bits(o[:, 2:]), _bits(base[:, 2:]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (48, 80))
def test_decode_padded_head_dims(gpu, d, dtype):
    from exploring_flash_attention_amd import ops
    for causal, lens in itertools.product((False, True), (None, (200, 37))):
        q, k, v = _inputs(2, 4, 2, 3, 200, d, dtype)
        o = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu), seqlens_k=_sl(lens, gpu), causal=causal)
        assert tuple(o.shape) == (2, 4, 3, d)
        _gate(o, _ref(2, 4, 2, 3, 200, d, dtype, causal, lens), dtype, f"padded d={d} causal={causal} lens={lens}")


@pytest.mark.gpu
def test_decode_workspace_reuse_and_out(gpu):
    from exploring_flash_attention_amd import ops
    dtype = torch.bfloat16
    q, k, v = _inputs(2, 4, 2, 3, 1041, 128, dtype)
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    splits, _, nbytes = ops.decode_plan(2, 4, 2, 3, 1041, 128, 5, dtype)
    assert splits == 5 and nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)  # never reset by the caller
    lens = _sl((37, 1041), gpu)
    out = torch.full((2, 4, 3, 128), float("nan"), dtype=dtype, device=gpu)
    a = ops.attention_decode(qd, kd, vd, seqlens_k=lens, num_splits=5, workspace=ws, out=out)
    assert a is out
    first = _bits(a).clone()
    b = ops.attention_decode(qd, kd, vd, seqlens_k=lens, num_splits=5, workspace=ws)
    c = ops.attention_decode(qd, kd, vd, seqlens_k=lens, num_splits=5)
    assert torch.equal(first, _bits(b)) and torch.equal(first, _bits(c))
    _gate(out, _ref(2, 4, 2, 3, 1041, 128, dtype, True, (37, 1041)), dtype, "workspace reuse / out=")
    with pytest.raises(ValueError, match="workspace too small"):
        ops.attention_decode(qd, kd, vd, num_splits=5, workspace=ws[:nbytes - 1])
    # a non-contiguous out is honoured through a copy
    wide = torch.zeros((2, 4, 3, 256), dtype=dtype, device=gpu)
    o2 = ops.attention_decode(qd, kd, vd, seqlens_k=lens, num_splits=5, out=wide[..., :128])
    assert torch.equal(_bits(o2.contiguous()), first) and (wide[..., 128:] == 0).all()
    # empty inputs: no launch
    with ops.launched_kernels() as kl:
        e = ops.attention_decode(qd[:0], kd[:0], vd[:0])
        z = ops.attention_decode(qd, kd[:, :, :0], vd[:, :, :0])
    assert kl == [] and e.numel() == 0 and tuple(z.shape) == (2, 4, 3, 128) and (z == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_decode_full_chip_auto_plan(gpu, dtype):
    from exploring_flash_attention_amd import ops
    B, H, Hkv, Lq, Lk, d = 2, 8, 2, 1, 8192, 128
    q, k, v = _inputs(B, H, Hkv, Lq, Lk, d, dtype)
    splits = ops.decode_plan(B, H, Hkv, Lq, Lk, d, None, dtype)[0]
    assert splits > 1
    with ops.launched_kernels() as kl:
        o = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu))
    assert f"[grid {B * Hkv * splits}]" in kl[0], kl
    _gate(o, _ref(B, H, Hkv, Lq, Lk, d, dtype, True), dtype, f"full chip, {splits} splits")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_decode_wide_row_tiles(gpu, d, dtype):
    """R = 32 and R = 64 (the 32- and 64-row instantiations), causal over a split boundary."""
    from exploring_flash_attention_amd import ops
    for (H, Hkv, Lq), causal in itertools.product(((8, 2, 8), (8, 1, 8), (2, 2, 64), (4, 2, 13)), (False, True)):
        q, k, v = _inputs(2, H, Hkv, Lq, 200, d, dtype)
        for ns, lens in itertools.product((None, 3), (None, (200, 37), (130, 5))):
            with ops.launched_kernels() as kl:
                o = ops.attention_decode(q.to(gpu), k.to(gpu), v.to(gpu), seqlens_k=_sl(lens, gpu), causal=causal, num_splits=ns)
            R = H // Hkv * Lq
            assert f"<{16 if R <= 16 else 32 if R <= 32 else 64} rows>" in kl[0], kl
            _gate(o, _ref(2, H, Hkv, Lq, 200, d, dtype, causal, lens), dtype,
                  f"R={R} H{H}/{Hkv} Lq{Lq} d{d} causal={causal} lens={lens} ns={ns}", quiet=True)
