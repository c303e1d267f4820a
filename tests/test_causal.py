"""Causal masking of the fused forward (fa_fwd_v1_causal, ops.attention_v1(causal=True)): row i
of every head attends to keys 0..i.

CPU part: the entry's argument checks (no launch), the host-tensor refusal, and this file's own
fp64 causal reference against torch's scaled_dot_product_attention(is_causal=True).

GPU part: fp64 reference on the SAME storage-rounded inputs the kernel sees.  Gate, per element,
    |out - ref| <= A + eps * |ref|
plus the project's mean_rel bound over |ref| > 1e-3, with (A, mean_rel) the build gate of
tests/test_gpu.py -- bf16 (6e-3, 1e-2), fp16 (2e-3, 3e-3) -- and eps the storage type's half-ulp
(2^-8 bf16, 2^-11 fp16).  The plain max_abs gate cannot serve here: the early causal rows are
averages of one or two V rows, |O| up to about 3, and rounding such an output to bf16 alone is
up to 7.8e-3.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import exploring_flash_attention_amd._lib as L

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x10000)

GATE = {torch.bfloat16: (6e-3, 1e-2, 2.0 ** -8), torch.float16: (2e-3, 3e-3, 2.0 ** -11)}
DTYPES = (torch.bfloat16, torch.float16)
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def causal_ref(q, k, v, scale=None):
    """fp64 causal attention over the last two dims ([..., L, d]): row i sees keys 0..i."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    L_, d = q.shape[-2:]
    s = (q @ np.swapaxes(k, -1, -2)) * (1.0 / np.sqrt(d) if scale is None else scale)
    s = np.where(np.tril(np.ones((L_, L_), bool)), s, -np.inf)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return (p / p.sum(axis=-1, keepdims=True)) @ v


# ----------------------------------------------------------------------------------------
# CPU: argument checks, host refusal, the reference itself
# ----------------------------------------------------------------------------------------


def test_causal_entry_argument_checks():
    lib = L.lib()
    fn = lib.fa_fwd_v1_causal
    st = fn(NULL, NULL, NULL, NULL, 1, 1, 64, 128, 0.1, L.FA_DTYPE_BF16, NULL)
    assert st == L.FA_ERR_INVALID_ARG and b"null" in lib.fa_last_error()
    for i in range(4):  # each pointer on its own
        ptrs = [FAKE] * 4
        ptrs[i] = NULL
        assert fn(*ptrs, 1, 1, 64, 128, 0.1, L.FA_DTYPE_BF16, NULL) == L.FA_ERR_INVALID_ARG
    st = fn(FAKE, FAKE, FAKE, FAKE, 1, 1, 64, 96, 0.1, L.FA_DTYPE_BF16, NULL)
    assert st == L.FA_ERR_UNSUPPORTED and b"d=96" in lib.fa_last_error()
    st = fn(FAKE, FAKE, FAKE, FAKE, 1, 1, 64, 384, 0.1, L.FA_DTYPE_BF16, NULL)
    assert st == L.FA_ERR_UNSUPPORTED and b"causal" in lib.fa_last_error() and b"384" in lib.fa_last_error()
    st = fn(FAKE, FAKE, FAKE, FAKE, 1, 1, 64, 128, 0.1, L.FA_DTYPE_FP64, NULL)
    assert st == L.FA_ERR_UNSUPPORTED and b"causal" in lib.fa_last_error() and b"FP64" in lib.fa_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        st = fn(FAKE, FAKE, FAKE, FAKE, 1, 1, 64, 128, bad, L.FA_DTYPE_BF16, NULL)
        assert st == L.FA_ERR_INVALID_ARG and b"softmax_scale" in lib.fa_last_error()
    st = fn(ctypes.c_void_p(0x10002), FAKE, FAKE, FAKE, 1, 1, 64, 128, 0.1, L.FA_DTYPE_BF16, NULL)
    assert st == L.FA_ERR_INVALID_ARG and b"aligned" in lib.fa_last_error()
    st = fn(FAKE, FAKE, FAKE, FAKE, 1, 0, 64, 128, 0.1, L.FA_DTYPE_BF16, NULL)
    assert st == L.FA_ERR_INVALID_ARG and b"positive" in lib.fa_last_error()


def test_causal_rejects_host_tensors():
    from exploring_flash_attention_amd import ops
    t = torch.zeros(1, 1, 64, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.attention_v1(t, t, t, causal=True)


def test_causal_reference_matches_torch_sdpa():
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 3, 37, 16, generator=g, dtype=torch.float64) for _ in range(3))
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True).numpy()
    got = causal_ref(q.numpy(), k.numpy(), v.numpy())
    assert np.abs(got - want).max() <= 1e-12
    # row 0 is V[0], and no row depends on a later key
    assert np.abs(got[..., 0, :] - v.numpy()[..., 0, :]).max() <= 1e-15
    k2, v2 = k.clone(), v.clone()
    k2[..., 20:, :] *= 50
    v2[..., 20:, :] *= 50
    assert np.array_equal(causal_ref(q.numpy(), k2.numpy(), v2.numpy())[..., :20, :], got[..., :20, :])


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _case(B, H, L_, d, dtype, seed=0, dist="normal"):
    """Seeded inputs (host, storage-rounded) and their fp64 causal reference, computed once and
    shared; nobody writes to them."""
    g = torch.Generator().manual_seed(seed)
    mk = (lambda: torch.randn(B, H, L_, d, generator=g)) if dist == "normal" else (
        lambda: torch.rand(B, H, L_, d, generator=g) * 2 - 1)
    q, k, v = (mk().to(dtype) for _ in range(3))
    ref = causal_ref(q.double().numpy(), k.double().numpy(), v.double().numpy())
    ref.setflags(write=False)
    return q, k, v, ref


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


def _lengths(d):
    # 1: a single row; 31: inside one wave; 64: one whole KV tile; 65: key tail inside the diagonal
    # tile; 128: one whole query tile (waves 0 and 1 wholly masked on the last tile); 129: second
    # query tile of one row; 200: two query tiles; 257, 384: three; d = 256 (32-key tiles, four
    # diagonal tiles): 96 and 160 in addition
    return (1, 31, 64, 65, 96, 128, 129, 160, 200, 257, 384) if d == 256 else (1, 31, 64, 65, 128, 129, 200, 257, 384)


SHAPES = [(d, L_) for d in (32, 64, 128, 256) for L_ in _lengths(d)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d,L_", SHAPES, ids=[f"d{d}-L{L_}" for d, L_ in SHAPES])
def test_causal_matches_fp64_reference(gpu, d, L_, dtype):
    from exploring_flash_attention_amd import ops
    q, k, v, ref = _case(2, 3, L_, d, dtype)
    o = ops.attention_v1(q.to(gpu), k.to(gpu), v.to(gpu), causal=True)
    assert o.dtype == dtype and tuple(o.shape) == (2, 3, L_, d)
    _gate(o, ref, dtype, f"causal d={d} L={L_} {IDS[dtype]}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_causal_uniform_inputs(gpu, dtype):
    """U[-1, 1] inputs (flat softmax rows: every visible key carries weight)."""
    from exploring_flash_attention_amd import ops
    for d, L_ in ((64, 200), (128, 130)):
        q, k, v, ref = _case(2, 3, L_, d, dtype, seed=5, dist="uniform")
        _gate(ops.attention_v1(q.to(gpu), k.to(gpu), v.to(gpu), causal=True), ref, dtype, f"uniform d={d} L={L_}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_causal_eight_query_tiles(gpu, dtype):
    """B1 H2 L1024 d128: eight query tiles per head under the heaviest-first order, the
    below-diagonal steady steps included."""
    from exploring_flash_attention_amd import ops
    q, k, v, ref = _case(1, 2, 1024, 128, dtype, seed=1)
    with ops.launched_kernels() as kl:
        o = ops.attention_v1(q.to(gpu), k.to(gpu), v.to(gpu), causal=True)
    assert kl == ["fa_fwd_kernel<final, causal> [grid 16]"], kl
    _gate(o, ref, dtype, f"eight tiles {IDS[dtype]}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_causal_no_leak_from_the_future(gpu, d, dtype):
    """K and V rows > j replaced by values 50x larger (finite: 0 * NaN would be NaN).  j = 127 is
    a query-tile boundary: rows 0..127 never load those keys and come out bitwise equal.  j = 100
    and j = 31 cut through a diagonal tile: rows <= j still meet the gate."""
    from exploring_flash_attention_amd import ops
    q, k, v, ref = _case(2, 3, 256, d, dtype, seed=2)
    qd = q.to(gpu)
    base = ops.attention_v1(qd, k.to(gpu), v.to(gpu), causal=True)
    _gate(base, ref, dtype, f"no-leak base d={d}")
    for j in (127, 100, 31):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, j + 1:] *= 50
        v2[:, :, j + 1:] *= 50
        assert torch.isfinite(k2.float()).all() and torch.isfinite(v2.float()).all()
        o = ops.attention_v1(qd, k2.to(gpu), v2.to(gpu), causal=True)
        if j == 127:
            assert torch.equal(o[:, :, :128], base[:, :, :128])
        _gate(o[:, :, :j + 1], ref[:, :, :j + 1], dtype, f"no-leak d={d} j={j}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (48, 80))
def test_causal_padded_head_dims(gpu, d, dtype):
    from exploring_flash_attention_amd import ops
    q, k, v, ref = _case(2, 3, 130, d, dtype, seed=4)
    with ops.launched_kernels() as kl:
        o = ops.attention_v1(q.to(gpu), k.to(gpu), v.to(gpu), causal=True)
    assert tuple(o.shape) == (2, 3, 130, d) and "causal" in kl[0]
    _gate(o, ref, dtype, f"padded d={d}")


@pytest.mark.gpu
def test_causal_views_out_and_labels(gpu):
    from exploring_flash_attention_amd import ops
    dtype = torch.bfloat16
    q, k, v, ref = _case(2, 3, 200, 64, dtype, seed=6)
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    with ops.launched_kernels() as kl:
        want = ops.attention_v1(qd, kd, vd, causal=True)
    assert len(kl) == 1 and "fa_fwd_kernel<final, causal>" in kl[0] and "[grid 12]" in kl[0]
    assert "causal" in L.last_kernels()
    _gate(want, ref, dtype, "contiguous")
    # [B, L, H, d] tensors viewed as [B, H, L, d]: the same result as their contiguous copies
    qs, ks, vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (qd, kd, vd))
    assert not qs.is_contiguous()
    assert torch.equal(ops.attention_v1(qs, ks, vs, causal=True), want)
    # out= is honoured (contiguous and strided)
    out = torch.empty_like(qd)
    assert ops.attention_v1(qd, kd, vd, out=out, causal=True) is out and torch.equal(out, want)
    outs = torch.empty(2, 200, 3, 64, dtype=dtype, device=gpu).transpose(1, 2)
    assert ops.attention_v1(qd, kd, vd, out=outs, causal=True) is outs and torch.equal(outs, want)
    # causal=False is today's path: bitwise equal to calling without the argument, no causal label
    with ops.launched_kernels() as kl:
        plain = ops.attention_v1(qd, kd, vd)
    assert "causal" not in kl[0] and "causal" not in L.last_kernels()
    assert torch.equal(ops.attention_v1(qd, kd, vd, causal=False), plain)
    assert not torch.equal(plain, want)
    # L = 0: the empty output, nothing launched
    e = torch.empty(2, 3, 0, 64, dtype=dtype, device=gpu)
    assert tuple(ops.attention_v1(e, e, e, causal=True).shape) == (2, 3, 0, 64)


@pytest.mark.gpu
def test_causal_package_surface_and_restrictions(gpu):
    import exploring_flash_attention_amd as fa
    from exploring_flash_attention_amd import ops
    dtype = torch.float16
    q, k, v, ref = _case(2, 3, 129, 128, dtype)
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    o = fa.flash_attention_v1(qd, kd, vd, causal=True)
    _gate(o, ref, dtype, "flash_attention_v1(causal=True)")
    assert torch.equal(o, ops.attention_v1(qd, kd, vd, causal=True))
    o2 = fa.flash_attention_v1(qd[1, 2], kd[1, 2], vd[1, 2], causal=True)  # device [L, d]
    _gate(o2[None, None], ref[1:2, 2:3], dtype, "flash_attention_v1 [L, d]")
    out = torch.empty_like(qd)
    fa.flash_attention_v1(qd, kd, vd, out, 2, 3, 129, 128, causal=True)  # launcher form
    assert torch.equal(out, o)
    assert torch.equal(fa.flash_attention_v1(qd, kd, vd, causal=False), fa.flash_attention_v1(qd, kd, vd))
    # fp16 host arrays run the fp16 kernel; float32 / float64 host arrays would run the fp64 one
    oh = fa.flash_attention_v1(q[0, 0].numpy(), k[0, 0].numpy(), v[0, 0].numpy(), causal=True)
    assert oh.dtype == np.float16 and np.array_equal(oh, o[0, 0].cpu().numpy())
    with pytest.raises(NotImplementedError, match="float64"):
        fa.flash_attention_v1(q[0, 0].double().numpy(), k[0, 0].double().numpy(), v[0, 0].double().numpy(),
                              causal=True)
    w = torch.zeros(1, 1, 64, 384, dtype=dtype, device=gpu)
    with pytest.raises(NotImplementedError, match="256"):
        ops.attention_v1(w, w, w, causal=True)
    f = torch.zeros(1, 1, 64, 64, dtype=torch.float64, device=gpu)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.attention_v1(f, f, f, causal=True)
