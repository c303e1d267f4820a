"""Grouped-query attention (fa_fwd_v1_gqa, ops.attention_v1 with [B, H_kv, L, d] K / V): query
head h reads K/V head h // G, G = H / H_kv -- the repeat_interleave(G, dim=1) convention.

CPU part: the export, the entry's argument checks (no launch), the Python refusals, this file's
fp64 reference against torch's scaled_dot_product_attention on expanded K / V, and a replay of
the kernels' work-item decode and K / V addressing (the K / V allocation is G times smaller
than an MHA one, so a b*h left on the K / V side reads out of bounds).

GPU part: fp64 reference on the SAME storage-rounded inputs under tests/test_causal.py's gate,
    |out - ref| <= A + eps * |ref|   and   mean_rel over |ref| > 1e-3,
bf16 (6e-3, 1e-2, 2^-8), fp16 (2e-3, 3e-3, 2^-11); and bit equality with the MHA call on
expanded K / V -- a workgroup's arithmetic does not depend on which head it is, so anything
short of bit equality is an addressing error.  Every GPU case has B = 2 and K / V heads that all
differ, so h % H_kv or a dropped batch term cannot pass.

The chain kernel (d = 128) needs at least as many query tiles as its persistent grid has
workgroups (2 per CU: 512), which no B = 2, H <= 6 case with a CPU reference reaches (L = 384
runs fa_fwd16_kernel there); it is reached by B2 H16 H_kv4 L2560 (640 tiles), checked bitwise
against the expanded form and, for three heads, against the fp64 reference.
"""
import ctypes
import functools
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
HEADS = ((4, 2), (6, 2), (4, 1))


def gqa_ref(q, k, v, causal=False, scale=None):
    """fp64 attention of q [B, H, L, d] over k, v [B, H_kv, L, d]: head h reads K/V head h // G."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    H, Hkv = q.shape[1], k.shape[1]
    assert H % Hkv == 0
    idx = np.arange(H) // (H // Hkv)
    k, v = k[:, idx], v[:, idx]
    L_, d = q.shape[-2:]
    s = (q @ np.swapaxes(k, -1, -2)) * (1.0 / np.sqrt(d) if scale is None else scale)
    if causal:
        s = np.where(np.tril(np.ones((L_, L_), bool)), s, -np.inf)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return (p / p.sum(axis=-1, keepdims=True)) @ v


# ----------------------------------------------------------------------------------------
# CPU: export, argument checks, refusals, the reference itself
# ----------------------------------------------------------------------------------------


def test_gqa_entry_is_exported_unmangled():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "fa_fwd_v1_gqa" in names
    assert "fa_fwd_v1_gqa" in L.SIGNATURES and L.FA_FWD_CAUSAL == 1
    assert L.lib().fa_version() == 0x000400


def test_gqa_entry_argument_checks():
    lib = L.lib()
    fn = lib.fa_fwd_v1_gqa
    BF = L.FA_DTYPE_BF16

    def err():
        return lib.fa_last_error()

    # pointers, alignment, sizes, scale: as fa_fwd_v1_scaled
    assert fn(NULL, NULL, NULL, NULL, 1, 4, 2, 64, 128, 0.1, 0, BF, NULL) == L.FA_ERR_INVALID_ARG and b"null" in err()
    for i in range(4):
        ptrs = [FAKE] * 4
        ptrs[i] = NULL
        assert fn(*ptrs, 1, 4, 2, 64, 128, 0.1, 0, BF, NULL) == L.FA_ERR_INVALID_ARG
    st = fn(ctypes.c_void_p(0x10002), FAKE, FAKE, FAKE, 1, 4, 2, 64, 128, 0.1, 0, BF, NULL)
    assert st == L.FA_ERR_INVALID_ARG and b"aligned" in err()
    st = fn(FAKE, FAKE, FAKE, FAKE, 1, 0, 2, 64, 128, 0.1, 0, BF, NULL)
    assert st == L.FA_ERR_INVALID_ARG and b"positive" in err()
    for flags in (0, L.FA_FWD_CAUSAL):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            st = fn(FAKE, FAKE, FAKE, FAKE, 1, 4, 2, 64, 128, bad, flags, BF, NULL)
            assert st == L.FA_ERR_INVALID_ARG and b"softmax_scale" in err()
        # H_kv: positive, at most H, a divisor of H
        for hkv in (0, -1, 8, 3):
            st = fn(FAKE, FAKE, FAKE, FAKE, 1, 4, hkv, 64, 128, 0.1, flags, BF, NULL)
            assert st == L.FA_ERR_INVALID_ARG and b"H_kv" in err(), (hkv, err())
        # head dims and types without a GQA kernel
        for d in (384, 512):
            st = fn(FAKE, FAKE, FAKE, FAKE, 1, 4, 2, 64, d, 0.1, flags, BF, NULL)
            assert st == L.FA_ERR_UNSUPPORTED and b"gqa" in err() and str(d).encode() in err()
        st = fn(FAKE, FAKE, FAKE, FAKE, 1, 4, 2, 64, 128, 0.1, flags, L.FA_DTYPE_FP64, NULL)
        assert st == L.FA_ERR_UNSUPPORTED and b"gqa" in err() and b"FP64" in err()
        st = fn(FAKE, FAKE, FAKE, FAKE, 1, 4, 2, 64, 96, 0.1, flags, BF, NULL)  # as fa_fwd_v1
        assert st == L.FA_ERR_UNSUPPORTED and b"d=96" in err()
    # unknown flag bits
    for flags in (2, 3, 0x80000000):
        st = fn(FAKE, FAKE, FAKE, FAKE, 1, 4, 2, 64, 128, 0.1, flags, BF, NULL)
        assert st == L.FA_ERR_INVALID_ARG and b"flags" in err()


def test_gqa_python_refusals(monkeypatch):
    import exploring_flash_attention_amd as fa
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    q = torch.zeros(1, 4, 64, 128, dtype=bf)
    kv = torch.zeros(1, 2, 64, 128, dtype=bf)
    with pytest.raises(ValueError, match="no CPU fallback"):  # host tensors: refused as ever
        ops.attention_v1(q, kv, kv)
    # float32 / float64 host arrays would run the fp64 kernels
    for dt in (np.float32, np.float64):
        with pytest.raises(NotImplementedError, match="GQA"):
            fa.flash_attention_v1(np.zeros((1, 4, 8, 16), dt), np.zeros((1, 2, 8, 16), dt), np.zeros((1, 2, 8, 16), dt))
    # the checks behind the device check, on host tensors (nothing is launched before they raise)
    monkeypatch.setattr(ops, "_check_tensor", lambda *a, **k: None)
    k3 = torch.zeros(1, 3, 64, 128, dtype=bf)
    for causal in (False, True):
        with pytest.raises(ValueError, match="multiple"):
            ops.attention_v1(q, k3, k3, causal=causal)
        with pytest.raises(NotImplementedError, match="GQA"):
            ops.attention_v1(q.double(), kv.double(), kv.double(), causal=causal)
        for d in (320, 384, 512):
            with pytest.raises(NotImplementedError, match="GQA"):
                ops.attention_v1(torch.zeros(1, 4, 8, d, dtype=bf), torch.zeros(1, 2, 8, d, dtype=bf),
                                 torch.zeros(1, 2, 8, d, dtype=bf), causal=causal)
    with pytest.raises(ValueError, match="same shape"):  # k and v must still agree
        ops.attention_v1(q, kv, k3)
    with pytest.raises(ValueError):  # and B, L, d with q
        ops.attention_v1(q, torch.zeros(1, 2, 32, 128, dtype=bf), torch.zeros(1, 2, 32, 128, dtype=bf))
    # every other operator keeps refusing mismatched head counts, and says where GQA lives
    # (the multi-GPU path checks its shards with ops._check_qkv(..., same_len=False))
    for call in (lambda: ops.attention_tiled_d(q, kv, kv), lambda: ops.attention_v2(q, kv, kv),
                 lambda: ops.attention_partial(q, kv, kv), lambda: ops._check_qkv(q, kv, kv, same_len=False)):
        with pytest.raises(ValueError, match="attention_v1 only"):
            call()


def test_gqa_reference_matches_torch_sdpa():
    B, H, Hkv, L_, d = 2, 6, 2, 37, 16
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B, H, L_, d, generator=g, dtype=torch.float64)
    k, v = (torch.randn(B, Hkv, L_, d, generator=g, dtype=torch.float64) for _ in range(2))
    ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    for causal in (False, True):
        want = torch.nn.functional.scaled_dot_product_attention(q, ke, ve, is_causal=causal).numpy()
        got = gqa_ref(q.numpy(), k.numpy(), v.numpy(), causal)
        assert np.abs(got - want).max() <= 1e-12, causal
    # heads 0..2 read K/V head 0 only
    k2, v2 = k.clone(), v.clone()
    k2[:, 1] *= 50
    v2[:, 1] *= 50
    assert np.array_equal(gqa_ref(q.numpy(), k2.numpy(), v2.numpy())[:, :3], gqa_ref(q.numpy(), k.numpy(), v.numpy())[:, :3])


# ----------------------------------------------------------------------------------------
# CPU: address replay of the shipped decode (fa_internal.hpp decode_item_gqa / gqa_kv_head,
# fa_fwd_gqa.hip's launch rule, fa_fwd16_chain.hpp's item lists)
# ----------------------------------------------------------------------------------------

KBQ = 128


def _xcd_remap(b, n):
    q, r = n >> 3, n & 7
    x, i = b & 7, b >> 3
    return np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + i


def _chain_items(nitems, grid):
    """Every work item the chain kernel's workgroups run, in (workgroup, position) order."""
    out = []
    iq, ir, nl = nitems >> 3, nitems & 7, grid >> 3
    for blk in range(grid):
        x, l = blk & 7, blk >> 3
        gstart = x * (iq + 1) if x < ir else ir * (iq + 1) + (x - ir) * iq
        gcnt = iq + (1 if x < ir else 0)
        nmine = (gcnt - l + nl - 1) // nl if l < gcnt else 0
        out.extend(gstart + l + nl * j for j in range(nmine))
    return np.asarray(out, dtype=np.int64)


def gqa_replay(B, H, Hkv, L_, d, causal, cus=256, kv_head=None):
    """Replay one fa_fwd_v1_gqa launch; returns the kernel family.  kv_head: the K/V head of
    flat query head bh (default: the shipped bh // G)."""
    G, BH = H // Hkv, B * H
    nqt = (L_ + KBQ - 1) // KBQ
    nblk = nqt * BH
    bk = 64 if d <= 128 else 32
    grid = 2 * cus // 8 * 8
    if not causal and d == 128 and L_ % 128 == 0 and L_ >= 256 and nblk >= grid >= 8:
        family, w = "chain", _chain_items(nblk, grid)
    else:
        family = "fwd16" if not causal and d == 128 and L_ % bk == 0 else "fwd"
        w = _xcd_remap(np.arange(nblk, dtype=np.int64), nblk)
    assert np.array_equal(np.sort(w), np.arange(nblk)), "work items are not a permutation of the grid"
    # decode_item_gqa: (b*h, query tile); causal: (K/V head, query tile longest first, head in group)
    if causal:
        g, rest = w % G, w // G
        qt, bh = nqt - 1 - rest % nqt, (rest // nqt) * G + g
    else:
        qt, bh = w % nqt, w // nqt
    assert np.array_equal(np.sort(bh * nqt + qt), np.arange(nblk)), "decode is not a bijection onto (b, h, qt)"
    b, h = bh // H, bh % H
    kvh = bh // G if kv_head is None else kv_head(bh)
    assert np.array_equal(kvh, b * Hkv + h // G), "K/V head is not h // G of batch b"
    # K / V tile descriptors against the [B, H_kv, L, d] allocation
    ROWB, nbytes = 2 * d, B * Hkv * L_ * d * 2
    kv_end = np.minimum((qt + 1) * KBQ, L_) if causal else np.full_like(qt, L_)
    ntiles = (kv_end + bk - 1) // bk
    base = 2 * (kvh * L_ * d)
    for t in range(int(ntiles.max())):
        live = t < ntiles
        valid = np.clip(kv_end - t * bk, 0, bk)
        start, length = base + t * bk * ROWB, valid * ROWB
        bad = live & (length > 0) & ((start < 0) | (start + length > nbytes))
        assert not bad.any(), f"K/V tile {t}: {int(bad.sum())} descriptors leave the {nbytes}-byte allocation"
    # Q and O of the tile stay in the [B, H, L, d] allocation
    q_rows = np.minimum(L_ - qt * KBQ, KBQ)
    q0 = 2 * (bh * L_ + qt * KBQ) * d
    assert (q_rows > 0).all() and (q0 >= 0).all() and (q0 + q_rows * ROWB <= BH * L_ * d * 2).all()
    return family


REPLAY_GRIDS = ((2, 4, 2, 384), (2, 6, 2, 200), (1, 4, 1, 129))


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("grid", REPLAY_GRIDS, ids=lambda g: "B%d-H%d-Hkv%d-L%d" % g)
def test_gqa_address_replay(grid, causal):
    fam = {d: gqa_replay(*grid, d, causal) for d in (32, 64, 128, 256)}
    if not causal:
        assert fam[128] == ("fwd16" if grid[3] % 64 == 0 else "fwd") and fam[64] == "fwd"


def test_gqa_address_replay_llm_shape():
    """B4 H32 H_kv8 L4096 d128: the chain kernel's item lists (4096 items on 512 workgroups), and
    the causal kernel's grid."""
    assert gqa_replay(4, 32, 8, 4096, 128, False) == "chain"
    assert gqa_replay(4, 32, 8, 4096, 128, True) == "fwd"
    assert gqa_replay(2, 16, 4, 2560, 128, False) == "chain"  # 640 items: more than one per workgroup


def test_gqa_replay_catches_an_mha_base():
    """The replay refuses the two mistakes it is there for: K / V addressed with the query's b*h
    (out of bounds), and h % H_kv (in bounds, the wrong head)."""
    with pytest.raises(AssertionError):
        gqa_replay(2, 4, 2, 384, 128, False, kv_head=lambda bh: bh)
    with pytest.raises(AssertionError, match="h // G"):
        gqa_replay(2, 4, 2, 384, 128, False, kv_head=lambda bh: (bh // 4) * 2 + bh % 2)
    with pytest.raises(AssertionError, match="h // G"):
        gqa_replay(2, 4, 2, 384, 128, False, kv_head=lambda bh: (bh % 4) // 2)  # batch term dropped


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _inputs(B, H, Hkv, L_, d, dtype, seed=0):
    """Seeded storage-rounded host inputs, computed once and shared; nobody writes to them."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L_, d, generator=g).to(dtype)
    k, v = (torch.randn(B, Hkv, L_, d, generator=g).to(dtype) for _ in range(2))
    return q, k, v


@functools.lru_cache(maxsize=None)
def _ref(B, H, Hkv, L_, d, dtype, causal, seed=0):
    q, k, v = _inputs(B, H, Hkv, L_, d, dtype, seed)
    ref = gqa_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), causal)
    ref.setflags(write=False)
    return ref


def _gate(out, ref, dtype, label=""):
    out = out.float().cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert np.isfinite(out).all(), label
    A, mean_rel_tol, eps = GATE[dtype]
    err = np.abs(out - ref)
    bound = A + eps * np.abs(ref)
    worst = float((err / bound).max()) if err.size else 0.0
    big = np.abs(ref) > 1e-3
    mean_rel = float((err[big] / np.abs(ref[big])).mean()) if big.any() else 0.0
    print(f"{label}: max_abs={err.max() if err.size else 0.0:.3e} worst err/bound={worst:.3f} mean_rel={mean_rel:.3e}")
    assert worst <= 1.0, (label, worst, float(err.max()))
    assert mean_rel <= mean_rel_tol, (label, mean_rel)
    return worst


def _expand(t, G):
    return t.repeat_interleave(G, dim=1)


SHAPES = [(d, L_) for d in (32, 64, 128, 256) for L_ in (1, 65, 128, 200, 384)]


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d,L_", SHAPES, ids=[f"d{d}-L{L_}" for d, L_ in SHAPES])
def test_gqa_matches_fp64_reference(gpu, d, L_, dtype, causal):
    from exploring_flash_attention_amd import ops
    worst = 0.0
    for H, Hkv in HEADS:
        q, k, v = _inputs(2, H, Hkv, L_, d, dtype)
        with ops.launched_kernels() as kl:
            o = ops.attention_v1(q.to(gpu), k.to(gpu), v.to(gpu), causal=causal)
        assert o.dtype == dtype and tuple(o.shape) == (2, H, L_, d)
        assert len(kl) == 1 and ", gqa>" in kl[0] and ("causal" in kl[0]) == causal, kl
        worst = max(worst, _gate(o, _ref(2, H, Hkv, L_, d, dtype, causal), dtype,
                                 f"gqa H{H}/{Hkv} d={d} L={L_} {IDS[dtype]} causal={causal}"))
    print(f"worst err/bound over the head counts: {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_gqa_kernel_families(gpu, dtype):
    """The d = 128 cases reach all four GQA kernels under the launch rule of the MHA call."""
    from exploring_flash_attention_amd import ops
    seen = {}
    for (B, H, Hkv, L_), causal in (((2, 4, 2, 128), False), ((2, 4, 2, 384), False), ((2, 4, 2, 200), False),
                                    ((2, 16, 4, 2560), False), ((2, 4, 2, 384), True)):
        q, k, v = (t.to(gpu) for t in _inputs(B, H, Hkv, L_, 128, dtype))
        with ops.launched_kernels() as kl:
            ops.attention_v1(q, k, v, causal=causal)
        with ops.launched_kernels() as kl_mha:
            ops.attention_v1(q, _expand(k, H // Hkv), _expand(v, H // Hkv), causal=causal)
        assert len(kl) == 1 and kl[0] == kl_mha[0].replace(">", ", gqa>"), (kl, kl_mha)
        seen[(L_, causal)] = kl[0].split(" [")[0]
    assert seen == {(128, False): "fa_fwd16_kernel<final, gqa>", (384, False): "fa_fwd16_kernel<final, gqa>",
                    (200, False): "fa_fwd_kernel<final, gqa>", (2560, False): "fa_fwd16_chain_kernel<final, gqa>",
                    (384, True): "fa_fwd_kernel<final, causal, gqa>"}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d,L_", ((64, 200), (128, 384), (256, 160)))
def test_gqa_bitwise_equals_expanded_kv(gpu, d, L_, dtype, causal):
    from exploring_flash_attention_amd import ops
    for H, Hkv in HEADS:
        q, k, v = (t.to(gpu) for t in _inputs(2, H, Hkv, L_, d, dtype))
        o = ops.attention_v1(q, k, v, causal=causal)
        want = ops.attention_v1(q, _expand(k, H // Hkv), _expand(v, H // Hkv), causal=causal)
        assert torch.equal(o, want), (H, Hkv, float((o.float() - want.float()).abs().max()))


@pytest.mark.gpu
def test_gqa_chain_kernel_several_items_per_workgroup(gpu):
    """B2 H16 H_kv4 L2560 d128 bf16: 640 items on the chain kernel's 512-workgroup grid.  Bitwise
    against the expanded form; heads (0, 0), (1, 7), (1, 15) also against the fp64 reference."""
    from exploring_flash_attention_amd import ops
    dtype = torch.bfloat16
    q, k, v = _inputs(2, 16, 4, 2560, 128, dtype, seed=3)
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    with ops.launched_kernels() as kl:
        o = ops.attention_v1(qd, kd, vd)
    assert kl == ["fa_fwd16_chain_kernel<final, gqa> [grid 512]"], kl
    with ops.launched_kernels() as kl:
        want = ops.attention_v1(qd, _expand(kd, 4), _expand(vd, 4))
    assert kl == ["fa_fwd16_chain_kernel<final> [grid 512]"], kl
    assert torch.equal(o, want)
    for b, h in ((0, 0), (1, 7), (1, 15)):
        ref = gqa_ref(q[b:b + 1, h:h + 1].double().numpy(), k[b:b + 1, h // 4:h // 4 + 1].double().numpy(),
                      v[b:b + 1, h // 4:h // 4 + 1].double().numpy())
        _gate(o[b:b + 1, h:h + 1], ref, dtype, f"chain b={b} h={h}")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_gqa_entry_with_all_heads_is_the_mha_entry(gpu, causal):
    """H_kv == H through fa_fwd_v1_gqa (ctypes): the kernels, labels and bits of fa_fwd_v1_scaled /
    fa_fwd_v1_causal."""
    lib = L.lib()
    for d, L_ in ((64, 200), (128, 128), (128, 200)):
        q, k, v = (t.to(gpu) for t in _inputs(2, 4, 4, L_, d, torch.bfloat16, seed=2))
        o1, o2 = torch.empty_like(q), torch.empty_like(q)
        stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        mha = lib.fa_fwd_v1_causal if causal else lib.fa_fwd_v1_scaled
        L.check(mha(ptr(q), ptr(k), ptr(v), ptr(o1), 2, 4, L_, d, 0.11, L.FA_DTYPE_BF16, stream))
        want_label = L.last_kernels()
        L.check(lib.fa_fwd_v1_gqa(ptr(q), ptr(k), ptr(v), ptr(o2), 2, 4, 4, L_, d, 0.11,
                                  L.FA_FWD_CAUSAL if causal else 0, L.FA_DTYPE_BF16, stream))
        assert L.last_kernels() == want_label and "gqa" not in want_label
        assert torch.equal(o1, o2)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d,L_", ((64, 200), (128, 384)))
def test_gqa_group_isolation(gpu, d, L_, causal):
    """K/V head 1 of both batches scaled by 50: the query heads of group 0 come out bitwise
    unchanged, those of group 1 do not."""
    from exploring_flash_attention_amd import ops
    dtype = torch.bfloat16
    q, k, v = (t.to(gpu) for t in _inputs(2, 4, 2, L_, d, dtype, seed=4))
    base = ops.attention_v1(q, k, v, causal=causal)
    k2, v2 = k.clone(), v.clone()
    k2[:, 1] *= 50
    v2[:, 1] *= 50
    assert torch.isfinite(k2.float()).all() and torch.isfinite(v2.float()).all()
    o = ops.attention_v1(q, k2, v2, causal=causal)
    assert torch.equal(o[:, :2], base[:, :2])
    assert not torch.equal(o[:, 2:], base[:, 2:])
    for b in (0, 1):
        assert not torch.equal(o[b, 2], base[b, 2]) and not torch.equal(o[b, 3], base[b, 3])


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (48, 80))
def test_gqa_padded_head_dims(gpu, d, dtype, causal):
    from exploring_flash_attention_amd import ops
    q, k, v = _inputs(2, 4, 2, 130, d, dtype, seed=5)
    with ops.launched_kernels() as kl:
        o = ops.attention_v1(q.to(gpu), k.to(gpu), v.to(gpu), causal=causal)
    assert tuple(o.shape) == (2, 4, 130, d) and "gqa" in kl[0]
    _gate(o, _ref(2, 4, 2, 130, d, dtype, causal, seed=5), dtype, f"padded d={d} causal={causal}")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_gqa_views_out_and_package_surface(gpu, causal):
    import exploring_flash_attention_amd as fa
    from exploring_flash_attention_amd import ops
    dtype = torch.float16
    B, H, Hkv, L_, d = 2, 6, 2, 200, 64
    q, k, v = _inputs(B, H, Hkv, L_, d, dtype, seed=6)
    ref = _ref(B, H, Hkv, L_, d, dtype, causal, seed=6)
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    want = ops.attention_v1(qd, kd, vd, causal=causal)
    _gate(want, ref, dtype, "contiguous")
    # [B, L, H, d] tensors viewed as [B, H, L, d]
    qs, ks, vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (qd, kd, vd))
    assert not qs.is_contiguous() and not ks.is_contiguous()
    o = ops.attention_v1(qs, ks, vs, causal=causal)
    _gate(o, ref, dtype, "transposed views")
    assert torch.equal(o, want)
    # out= is honoured (contiguous and strided)
    out = torch.empty_like(qd)
    assert ops.attention_v1(qd, kd, vd, out=out, causal=causal) is out and torch.equal(out, want)
    outs = torch.empty(B, L_, H, d, dtype=dtype, device=gpu).transpose(1, 2)
    assert ops.attention_v1(qd, kd, vd, out=outs, causal=causal) is outs and torch.equal(outs, want)
    # the package surface: device tensors, the launcher form, float16 host arrays
    assert torch.equal(fa.flash_attention_v1(qd, kd, vd, causal=causal), want)
    out2 = torch.empty_like(qd)
    fa.flash_attention_v1(qd, kd, vd, out2, B, H, L_, d, causal=causal)
    assert torch.equal(out2, want)
    oh = fa.flash_attention_v1(q.numpy(), k.numpy(), v.numpy(), causal=causal)
    assert oh.dtype == np.float16 and np.array_equal(oh, want.cpu().numpy())
    # L = 0: the empty output, nothing launched
    e = torch.empty(B, H, 0, d, dtype=dtype, device=gpu)
    ekv = torch.empty(B, Hkv, 0, d, dtype=dtype, device=gpu)
    assert tuple(ops.attention_v1(e, ekv, ekv, causal=causal).shape) == (B, H, 0, d)


@pytest.mark.gpu
def test_gqa_device_refusals(gpu):
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    q = torch.zeros(2, 4, 64, 64, dtype=bf, device=gpu)
    kv = torch.zeros(2, 2, 64, 64, dtype=bf, device=gpu)
    k3 = torch.zeros(2, 3, 64, 64, dtype=bf, device=gpu)
    with pytest.raises(ValueError, match="multiple"):
        ops.attention_v1(q, k3, k3)
    with pytest.raises(NotImplementedError, match="GQA"):
        ops.attention_v1(q.double(), kv.double(), kv.double())
    w, wkv = torch.zeros(1, 4, 64, 384, dtype=bf, device=gpu), torch.zeros(1, 2, 64, 384, dtype=bf, device=gpu)
    with pytest.raises(NotImplementedError, match="GQA"):
        ops.attention_v1(w, wkv, wkv)
    for call in (lambda: ops.attention_tiled_d(q, kv, kv), lambda: ops.attention_v2(q, kv, kv),
                 lambda: ops.attention_partial(q, kv, kv)):
        with pytest.raises(ValueError, match="attention_v1 only"):
            call()
