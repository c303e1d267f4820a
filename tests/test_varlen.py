"""Variable-length (token-packed) prefill attention: fa_fwd_varlen / ops.attention_varlen.

q and o are [T, H, d], k and v [T, H_kv, d]; an int32 cu_seqlens [B + 1] on the device says which
token rows belong to which sequence; each sequence attends to its own keys only, causal or not.

CPU part: the entry's argument checks (no launch), the Python-side checks, this file's fp64
reference against torch's scaled_dot_product_attention, and a NumPy replay of the kernel's item
decode, length clamps and descriptor arithmetic (csrc/fa_fwd_kernel.hpp, VARLEN) for whole grids:
the decode is a bijection, every Q and K/V descriptor of a running item lies inside its
allocation and inside its own sequence's rows, and the stored O rows are disjoint and exactly the
rows below each sequence's length -- for ragged, empty, truncated, strided and corrupt inputs.

GPU part: fp64 reference on the SAME storage-rounded inputs the kernel sees, under the gate of
tests/test_causal.py: per element |out - ref| <= A + eps * |ref| plus the mean_rel bound over
|ref| > 1e-3, bf16 (6e-3, 1e-2, 2^-8), fp16 (2e-3, 3e-3, 2^-11) -- the early causal rows and the
short sequences are averages of a few V rows, so |O| reaches about 3 and the plain max_abs gate
is below the rounding of such an output.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import exploring_flash_attention_amd._lib as L

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x10000)

GATE = {torch.bfloat16: (6e-3, 1e-2, 2.0 ** -8), torch.float16: (2e-3, 3e-3, 2.0 ** -11)}
DTYPES = (torch.bfloat16, torch.float16)
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}
KBQ = 128  # query rows per workgroup (fa_internal.hpp kBQ)
SENTINEL = -1024.0  # exact in bf16 and fp16, far outside any attention output of these inputs


def varlen_ref(q, k, v, cu, max_seqlen, causal):
    """fp64 reference.  q [T, H, d], k / v [T, H_kv, d], cu a valid (monotonic, within T) offset
    list.  Returns (o, owned): o [T, H, d] with NaN in the rows of no sequence, owned [T] bool.
    Sequence b is rows cu[b] : cu[b] + min(len_b, max_seqlen); head h reads K/V head h // G; with
    `causal` position p sees keys 0..p."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    T, H, d = q.shape
    G = H // k.shape[1]
    o = np.full((T, H, d), np.nan)
    owned = np.zeros(T, bool)
    for b in range(len(cu) - 1):
        s, n = int(cu[b]), min(int(cu[b + 1]) - int(cu[b]), int(max_seqlen))
        if n <= 0:
            continue
        owned[s:s + n] = True
        for h in range(H):
            sc = (q[s:s + n, h] @ k[s:s + n, h // G].T) / np.sqrt(d)
            if causal:
                sc = np.where(np.tril(np.ones((n, n), bool)), sc, -np.inf)
            p = np.exp(sc - sc.max(axis=-1, keepdims=True))
            o[s:s + n, h] = (p / p.sum(axis=-1, keepdims=True)) @ v[s:s + n, h // G]
    return o, owned


# ----------------------------------------------------------------------------------------
# CPU: the C entry's argument checks, the export, the Python-side checks, the reference
# ----------------------------------------------------------------------------------------


def _call(fn, q=FAKE, k=FAKE, v=FAKE, o=FAKE, cu=FAKE, B=2, T=300, msl=200, H=4, Hkv=2, d=128, qs=None, kvs=None,
          os_=None, scale=0.1, flags=0, dtype=L.FA_DTYPE_BF16):
    return fn(q, k, v, o, cu, B, T, msl, H, Hkv, d, qs, kvs, os_, scale, flags, dtype, NULL)


def test_varlen_entry_argument_checks():
    lib = L.lib()
    fn = lib.fa_fwd_varlen
    err = lib.fa_last_error
    for name in ("q", "k", "v", "o"):  # each tensor pointer on its own
        assert _call(fn, **{name: NULL}) == L.FA_ERR_INVALID_ARG and b"null" in err()
    assert _call(fn, cu=NULL) == L.FA_ERR_INVALID_ARG and b"cu_seqlens" in err()
    assert _call(fn, cu=ctypes.c_void_p(0x10002)) == L.FA_ERR_INVALID_ARG and b"cu_seqlens" in err()
    assert _call(fn, q=ctypes.c_void_p(0x10002)) == L.FA_ERR_INVALID_ARG and b"aligned" in err()
    for Hkv in (3, 0, 8, -1):
        assert _call(fn, Hkv=Hkv) == L.FA_ERR_INVALID_ARG and b"H_kv" in err()
    for flags in (2, 3, 0x80000000):
        assert _call(fn, flags=flags) == L.FA_ERR_INVALID_ARG and b"flags" in err()
    for d in (96, 16, 384, 512):
        assert _call(fn, d=d) == L.FA_ERR_UNSUPPORTED and f"d={d}".encode() in err()
    assert _call(fn, dtype=L.FA_DTYPE_FP64) == L.FA_ERR_UNSUPPORTED and b"varlen" in err() and b"FP64" in err()
    assert _call(fn, dtype=17) == L.FA_ERR_UNSUPPORTED
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(fn, scale=bad) == L.FA_ERR_INVALID_ARG and b"softmax_scale" in err()
    for msl in (0, -5):
        assert _call(fn, msl=msl) == L.FA_ERR_INVALID_ARG and b"max_seqlen" in err()
    for B in (0, -1):
        assert _call(fn, B=B) == L.FA_ERR_INVALID_ARG and b"B=" in err()
    assert _call(fn, T=-1) == L.FA_ERR_INVALID_ARG and b"total_tokens" in err()
    assert _call(fn, H=0) == L.FA_ERR_INVALID_ARG
    # grid = B * H * ceil(max_seqlen / 128) must stay below 2^31
    assert _call(fn, B=1 << 20, H=1 << 10, Hkv=1 << 10, T=1 << 30, msl=1 << 10) == L.FA_ERR_UNSUPPORTED
    assert b"grid" in err()
    assert _call(fn, B=1 << 24, H=128, Hkv=128, T=1 << 30, msl=1) == L.FA_ERR_UNSUPPORTED and b"grid" in err()
    assert _call(fn, T=1 << 31) == L.FA_ERR_UNSUPPORTED and b"total_tokens" in err()
    # strides {token, head}: positive multiples of 8 elements, token stride >= d and <= 2^20
    S2 = ctypes.c_int64 * 2
    for which in ("qs", "kvs", "os_"):
        for bad in ((1028, 128), (1024, 4), (0, 128), (1024, -8)):
            assert _call(fn, **{which: S2(*bad)}) == L.FA_ERR_INVALID_ARG and b"stride" in err()
        assert _call(fn, **{which: S2(64, 128)}) == L.FA_ERR_INVALID_ARG and b"token stride" in err()
        assert _call(fn, **{which: S2((1 << 20) + 8, 128)}) == L.FA_ERR_UNSUPPORTED and b"token stride" in err()
    # no tokens: FA_OK, nothing launched (the pointers are fakes)
    assert _call(fn, T=0) == L.FA_OK and lib.fa_last_kernels() == b""


def test_varlen_is_declared_and_exported():
    import exploring_flash_attention_amd as fa
    from exploring_flash_attention_amd import ops
    assert "fa_fwd_varlen" in L.SIGNATURES and len(L.SIGNATURES["fa_fwd_varlen"][1]) == 18
    assert fa.attention_varlen is ops.attention_varlen and "attention_varlen" in fa.__all__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fa_mi355x.h")) as f:
        assert "int fa_fwd_varlen(" in f.read()


def test_varlen_python_side_checks():
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    q, kv = torch.zeros(10, 4, 64, dtype=bf), torch.zeros(10, 2, 64, dtype=bf)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.attention_varlen(q, kv, kv, cu, 6)
    with pytest.raises(ValueError, match="cu_seqlens must be an int32"):
        ops.attention_varlen(q, kv, kv, cu.long(), 6)
    with pytest.raises(ValueError, match="cu_seqlens must be an int32"):
        ops.attention_varlen(q, kv, kv, cu.reshape(1, 3), 6)
    with pytest.raises(ValueError, match="cu_seqlens must be an int32"):
        ops.attention_varlen(q, kv, kv, torch.zeros(0, dtype=torch.int32), 6)
    with pytest.raises(TypeError, match="cu_seqlens"):
        ops.attention_varlen(q, kv, kv, [0, 4, 10], 6)
    with pytest.raises(ValueError, match="not a multiple of H_kv"):
        ops.attention_varlen(q, torch.zeros(10, 3, 64, dtype=bf), torch.zeros(10, 3, 64, dtype=bf), cu, 6)
    with pytest.raises(ValueError, match="3-D"):
        ops.attention_varlen(q[None], kv, kv, cu, 6)
    with pytest.raises(ValueError, match="disagree"):
        ops.attention_varlen(q, kv[:9], kv[:9], cu, 6)
    with pytest.raises(ValueError, match="same shape"):
        ops.attention_varlen(q, kv, kv[:, :1], cu, 6)


def test_varlen_reference_matches_torch_sdpa():
    g = torch.Generator().manual_seed(11)
    lens = (5, 0, 37, 1, 20)
    cu = np.concatenate([[0], np.cumsum(lens)])
    T, H, Hkv, d = int(cu[-1]) + 3, 4, 2, 16
    q = torch.randn(T, H, d, generator=g, dtype=torch.float64)
    k, v = (torch.randn(T, Hkv, d, generator=g, dtype=torch.float64) for _ in range(2))
    for causal in (False, True):
        got, owned = varlen_ref(q.numpy(), k.numpy(), v.numpy(), cu, 64, causal)
        assert owned.sum() == sum(lens) and not owned[int(cu[-1]):].any() and np.isnan(got[~owned]).all()
        for b, n in enumerate(lens):
            if n == 0:
                continue
            s = int(cu[b])
            qs = q[s:s + n].transpose(0, 1)
            ks, vs = (t[s:s + n].transpose(0, 1).repeat_interleave(H // Hkv, dim=0) for t in (k, v))
            want = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, is_causal=causal)
            assert np.abs(got[s:s + n] - want.transpose(0, 1).numpy()).max() <= 1e-12
    # truncation to max_seqlen: the sequence's first rows only, attending to those rows only
    got, owned = varlen_ref(q.numpy(), k.numpy(), v.numpy(), cu, 10, False)
    s = int(cu[2])
    assert owned[s:s + 10].all() and not owned[s + 10:s + 37].any()
    alone, _ = varlen_ref(q.numpy()[s:s + 10], k.numpy()[s:s + 10], v.numpy()[s:s + 10], [0, 10], 10, False)
    assert np.array_equal(got[s:s + 10], alone)


# ----------------------------------------------------------------------------------------
# CPU: address replay of the VARLEN kernel (csrc/fa_fwd_kernel.hpp) for whole grids
# ----------------------------------------------------------------------------------------


def bk_for(d):
    return 64 if d <= 128 else 32


def xcd_remap(b, n):
    q, r = n >> 3, n & 7
    x, i = b & 7, b >> 3
    return np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + i


class Alloc:
    """A buffer [lo, hi) in bytes relative to the pointer the kernel gets."""

    def __init__(self, name, nbytes, ptr_off=0):
        self.name, self.lo, self.hi = name, -ptr_off, nbytes - ptr_off

    def check(self, start, length, what):
        assert length > 0 and self.lo <= start and start + length <= self.hi, (
            f"{what}: [{start}, {start + length}) leaves {self.name} [{self.lo}, {self.hi})")


def replay_varlen(cu, T, max_seqlen, H, Hkv, D, causal, strides, allocs, valid_cu=True, clamp=True):
    """Replay one fa_fwd_varlen launch: fa_capi.cpp's launch arguments, the kernel's decode, clamps
    and descriptors.  strides: ({token, head} of q, of k/v, of o) in elements.  Asserts (i)-(iii)
    of the module docstring; returns (running items, stored (token row, head) pairs)."""
    cu = np.asarray(cu, np.int64)
    B = len(cu) - 1
    msl = min(max_seqlen, T)                      # fa_capi.cpp
    nqt = (msl + KBQ - 1) // KBQ
    G = H // Hkv
    nblk = B * H * nqt
    assert 0 < nblk < 1 << 31
    blk = np.arange(nblk, dtype=np.int64)
    w = xcd_remap(blk, nblk)
    assert np.array_equal(np.sort(w), blk), "xcd_remap is not a bijection onto the grid"
    if causal:   # decode_item_gqa<true>: (K/V head, query tile longest first, head in group)
        g, rest = w % G, w // G
        qt, bh = nqt - 1 - rest % nqt, (rest // nqt) * G + g
    else:        # decode_item_gqa<false>: (b*h, query tile)
        qt, bh = w % nqt, w // nqt
    b, h = bh // H, bh % H
    assert b.min() >= 0 and b.max() < B and qt.min() >= 0 and qt.max() < nqt
    # (i) a bijection onto (sequence, head, query tile)
    assert np.array_equal(np.sort((b * H + h) * nqt + qt), blk), "decode is not a bijection"
    if causal:   # the G heads of a K/V head, equally long, are neighbours
        order = np.argsort(w)
        assert (np.diff((b * Hkv + h // G)[order].reshape(-1, G), axis=1) == 0).all()
        assert (np.diff(qt[order].reshape(-1, G), axis=1) == 0).all()
    c0, c1 = cu[b], cu[b + 1]
    if clamp:
        st = np.clip(c0, 0, T)
        n = np.clip(c1 - st, 0, np.minimum(T - st, msl))
    else:        # (test_replay_catches_a_missing_clamp)
        st, n = c0, np.minimum(c1 - c0, msl)
    assert ((st + n <= T) & (st >= 0) & (n >= 0)).all() or not clamp
    run = qt * KBQ < n                            # the others return before any barrier or DMA
    (qs, ks, os_), ROWB, bk = strides, 2 * D, bk_for(D)
    qrb, krb = 2 * qs[0], 2 * ks[0]
    stored = []
    items = 0
    for i in np.nonzero(run)[0]:
        items += 1
        sti, ni, qti, hi, bi = int(st[i]), int(n[i]), int(qt[i]), int(h[i]), int(b[i])
        lo_row, hi_row = sti, sti + ni            # the sequence's own rows
        if valid_cu:
            assert int(cu[bi]) <= lo_row and hi_row <= int(cu[bi + 1])
        # ---- Q descriptor: the tile's rows below the length
        q_tile0 = qti * KBQ
        q_rows = min(ni - q_tile0, KBQ)
        assert q_rows >= 1
        q_base = 2 * (sti * qs[0] + hi * qs[1]) + q_tile0 * qrb
        q_len = (q_rows - 1) * qrb + ROWB
        allocs["q"].check(q_base, q_len, "Q descriptor")
        first = (q_base - 2 * hi * qs[1]) // qrb
        last = (q_base + q_len - ROWB - 2 * hi * qs[1]) // qrb
        assert lo_row <= first and last < hi_row, "Q descriptor leaves its sequence"
        # ---- K / V tile descriptors of the key range
        nkv = min((qti + 1) * KBQ, ni) if causal else ni
        ntiles = (nkv + bk - 1) // bk
        k_head = 2 * (sti * ks[0] + (hi // G) * ks[1])
        for t in range(ntiles + 2):               # (two prefetches past the end: empty descriptors)
            valid = min(max(nkv - t * bk, 0), bk)
            if t >= ntiles:
                assert valid == 0
                continue
            assert valid >= 1
            base = k_head + t * bk * krb
            length = (valid - 1) * krb + ROWB
            for name in ("k", "v"):
                allocs[name].check(base, length, f"{name.upper()} tile {t}")
            kfirst = (base - 2 * (hi // G) * ks[1]) // krb
            klast = (base + length - ROWB - 2 * (hi // G) * ks[1]) // krb
            assert lo_row <= kfirst and klast < hi_row, "K/V descriptor leaves its sequence"
        # ---- O row stores: rows of the tile below the length
        for r in range(q_tile0, min(q_tile0 + KBQ, ni)):
            allocs["o"].check(2 * ((sti + r) * os_[0] + hi * os_[1]), ROWB, "O row")
            stored.append((bi, hi, r, sti + r))
    # (iii) distinct items store disjoint rows, together the rows < len_b of every (b, head)
    per_seq = {(bi, hi, r) for bi, hi, r, _ in stored}
    assert len(per_seq) == len(stored), "two items store the same row"
    blen = {}
    for bi, sti, ni in zip(b.tolist(), st.tolist(), n.tolist()):
        blen[bi] = (sti, ni)
    want = {(bi, hi, r) for bi, (sti, ni) in blen.items() for hi in range(H) for r in range(ni)}
    assert per_seq == want, "stored rows are not exactly the rows below each length"
    if valid_cu:
        tok = {(row, hi) for _, hi, _, row in stored}
        assert len(tok) == len(stored), "two sequences store the same token row"
        assert all(row < int(cu[-1]) for row, _ in tok)
    return items, stored


def _contig(T, H, Hkv, D, guard_rows=0):
    """Contiguous [T, H, d] / [T, H_kv, d] tensors (guard rows of the allocation past T)."""
    strides = ((H * D, D), (Hkv * D, D), (H * D, D))
    allocs = {"q": Alloc("q", 2 * (T + guard_rows) * H * D), "k": Alloc("k", 2 * (T + guard_rows) * Hkv * D),
              "v": Alloc("v", 2 * (T + guard_rows) * Hkv * D), "o": Alloc("o", 2 * (T + guard_rows) * H * D)}
    return strides, allocs


RAGGED = (1, 31, 64, 65, 0, 128, 129, 200, 257)


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("H,Hkv", ((4, 4), (4, 2), (4, 1)))
def test_replay_ragged_batch(H, Hkv, D, causal):
    lens = RAGGED + ((96, 160) if D == 256 else ())
    cu = np.concatenate([[0], np.cumsum(lens)])
    T = int(cu[-1]) + 70
    strides, allocs = _contig(T, H, Hkv, D)
    items, stored = replay_varlen(cu, T, 257, H, Hkv, D, causal, strides, allocs)
    assert items == H * sum((n + KBQ - 1) // KBQ for n in lens)
    assert len(stored) == H * sum(lens)


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_replay_zero_length_sequences(causal):
    lens = (0, 0, 130, 0, 5, 0)
    cu = np.concatenate([[0], np.cumsum(lens)])
    strides, allocs = _contig(int(cu[-1]), 8, 2, 128)
    items, _ = replay_varlen(cu, int(cu[-1]), 130, 8, 2, 128, causal, strides, allocs)
    assert items == 8 * 3
    # every sequence empty: a grid of items that all exit
    cu0 = np.zeros(5, np.int64)
    items, stored = replay_varlen(cu0, 64, 64, 8, 2, 128, causal, *_contig(64, 8, 2, 128))
    assert items == 0 and not stored


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("max_seqlen", (128, 100, 1))
def test_replay_max_seqlen_below_the_longest(max_seqlen, causal):
    cu = np.concatenate([[0], np.cumsum(RAGGED)])
    T = int(cu[-1])
    items, stored = replay_varlen(cu, T, max_seqlen, 4, 2, 64, causal, *_contig(T, 4, 2, 64))
    assert len(stored) == 4 * sum(min(n, max_seqlen) for n in RAGGED)
    assert max(r for _, _, r, _ in stored) == max_seqlen - 1


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("D", (32, 128))
def test_replay_qkv_slice_layout(D, causal):
    """q, k, v as the three slices of one [T, (H + 2 H_kv) d] projection, o a strided view."""
    H, Hkv = 8, 2
    cu = np.concatenate([[0], np.cumsum(RAGGED)])
    T = int(cu[-1]) + 70
    W = (H + 2 * Hkv) * D
    strides = ((W, D), (W, D), (2 * H * D, 2 * D))
    allocs = {"q": Alloc("qkv", 2 * T * W, 0), "k": Alloc("qkv", 2 * T * W, 2 * H * D),
              "v": Alloc("qkv", 2 * T * W, 2 * (H + Hkv) * D), "o": Alloc("o", 2 * T * 2 * H * D)}
    # the last row's slice ends inside the buffer: q's last descriptor byte is below k's columns
    replay_varlen(cu, T, 257, H, Hkv, D, causal, strides, allocs)
    # the same with the views' exact extents as the allocation (a k slice ends with its last row)
    tight = {"q": Alloc("q", 2 * ((T - 1) * W + H * D)), "k": Alloc("k", 2 * ((T - 1) * W + Hkv * D)),
             "v": Alloc("v", 2 * ((T - 1) * W + Hkv * D)), "o": Alloc("o", 2 * ((T - 1) * 2 * H * D + (2 * H - 1) * D))}
    cu_all = np.concatenate([cu, [T]])  # a last sequence that ends with the last token row
    replay_varlen(cu_all, T, 257, H, Hkv, D, causal, strides, tight)


CORRUPT = {
    "decreasing": [0, 200, 100, 300, 50, 400],
    "negative": [-5, 100, -2 ** 31, 250, 260, 2 ** 31 - 1],
    "beyond T": [0, 100, 900, 5000, 2 ** 31 - 1, 450],
    "all huge": [2 ** 31 - 1] * 4,
    "all negative": [-2 ** 31, -1, -7, -2 ** 31],
}


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_replay_corrupt_cu_seqlens_stays_inside(name, causal):
    """Whatever cu_seqlens holds, the clamped (start, len) keep every descriptor and store inside
    rows [0, T): no guard rows in the allocations here."""
    T = 450
    for max_seqlen in (257, 10000):
        replay_varlen(CORRUPT[name], T, max_seqlen, 4, 2, 128, causal, *_contig(T, 4, 2, 128), valid_cu=False)


def test_replay_catches_a_missing_clamp():
    T = 450
    with pytest.raises(AssertionError, match="leaves"):
        replay_varlen(CORRUPT["beyond T"], T, 10000, 4, 2, 128, False, *_contig(T, 4, 2, 128), valid_cu=False,
                      clamp=False)


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------

GUARD = 70  # token rows of q / k / v / out past cu[B]: they belong to no sequence


def _lens(d):
    # 1: a single row; 31: inside one wave; 64: one whole KV tile; 65: a key tail in the diagonal
    # tile; 0: an empty sequence in the middle; 128: one whole query tile; 129: a second tile of one
    # row; 200: two tiles; 257: three; d = 256 (32-key tiles): 96 and 160 in addition
    return RAGGED + ((96, 160) if d == 256 else ())


@functools.lru_cache(maxsize=None)
def _batch(d, H, Hkv, dtype, seed=0, lens=None):
    """Seeded packed inputs (host, storage-rounded) with GUARD rows past cu[B]; shared, read-only."""
    lens = _lens(d) if lens is None else lens
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(cu[-1]) + GUARD
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(T, H, d, generator=g).to(dtype)
    k, v = (torch.randn(T, Hkv, d, generator=g).to(dtype) for _ in range(2))
    return q, k, v, cu, lens


@functools.lru_cache(maxsize=None)
def _ref(d, H, Hkv, dtype, causal, max_seqlen=257, seed=0, lens=None):
    q, k, v, cu, _ = _batch(d, H, Hkv, dtype, seed, lens)
    o, owned = varlen_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), cu, max_seqlen, causal)
    o.setflags(write=False)
    owned.setflags(write=False)
    return o, owned


def _cu_dev(cu, gpu):
    return torch.tensor(np.asarray(cu, np.int64).tolist(), dtype=torch.int32, device=gpu)


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


def _sentinel_out(q, gpu):
    return torch.full(tuple(q.shape), SENTINEL, dtype=q.dtype, device=gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (32, 64, 128, 256))
@pytest.mark.parametrize("H,Hkv", ((4, 4), (4, 2), (4, 1)), ids=("mha", "gqa2", "mqa"))
def test_varlen_matches_fp64_reference(gpu, H, Hkv, d, causal, dtype):
    """One ragged batch holding every edge at once; max_seqlen = 257, three query tiles."""
    from exploring_flash_attention_amd import ops
    q, k, v, cu, lens = _batch(d, H, Hkv, dtype)
    ref, owned = _ref(d, H, Hkv, dtype, causal)
    with ops.launched_kernels() as kl:
        o = ops.attention_varlen(q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu, gpu), 257, causal=causal)
    label = "fa_fwd_kernel<final, varlen" + (", causal" if causal else "") + (", gqa" if Hkv < H else "") + ">"
    assert kl == [f"{label} [grid {len(lens) * H * 3}]"], kl
    assert o.dtype == dtype and tuple(o.shape) == tuple(q.shape)
    _gate(o[torch.from_numpy(owned.copy())], ref[owned], dtype, f"varlen H{H}/{Hkv} d={d} causal={causal} {IDS[dtype]}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (64, 128))
def test_varlen_no_stray_stores(gpu, d, causal, dtype):
    """out preset to a sentinel: the GUARD rows past cu[B] and nothing else keep it; with
    max_seqlen = 128 the positions >= 128 keep it too and the rows below match the reference on
    the truncated sequences."""
    from exploring_flash_attention_amd import ops
    H, Hkv = 4, 2
    q, k, v, cu, lens = _batch(d, H, Hkv, dtype)
    qd, kd, vd, cud = q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu, gpu)
    for msl in (257, 128):
        ref, owned = _ref(d, H, Hkv, dtype, causal, msl)
        assert owned.sum() == sum(min(n, msl) for n in lens) and not owned[-GUARD:].any()
        out = _sentinel_out(q, gpu)
        assert ops.attention_varlen(qd, kd, vd, cud, msl, causal=causal, out=out) is out
        o = out.cpu()
        own = torch.from_numpy(owned.copy())
        assert (o[~own].float() == SENTINEL).all(), f"a row of no sequence was written (max_seqlen={msl})"
        assert (o[own].float() != SENTINEL).all(), f"an owned row was not written (max_seqlen={msl})"
        _gate(o[own], ref[owned], dtype, f"no-stray d={d} causal={causal} max_seqlen={msl}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_sequences_are_isolated(gpu, causal, dtype):
    """K and V of every other sequence (and of the guard rows) times 50, or NaN: a sequence's rows
    are bitwise unchanged."""
    from exploring_flash_attention_amd import ops
    d, H, Hkv = 128, 4, 2
    q, k, v, cu, lens = _batch(d, H, Hkv, dtype, seed=3)
    qd, cud = q.to(gpu), _cu_dev(cu, gpu)
    base = ops.attention_varlen(qd, k.to(gpu), v.to(gpu), cud, 257, causal=causal)
    for j in (0, 3, 6, 8):  # lengths 1, 65, 129, 257
        s, n = int(cu[j]), lens[j]
        for poison in ("x50", "nan"):
            k2, v2 = k.clone(), v.clone()
            for t in (k2, v2):
                keep = t[s:s + n].clone()
                if poison == "x50":
                    t *= 50
                else:
                    t.fill_(float("nan"))
                t[s:s + n] = keep
            o = ops.attention_varlen(qd, k2.to(gpu), v2.to(gpu), cud, 257, causal=causal)
            assert torch.equal(o[s:s + n], base[s:s + n]), (j, poison)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (64, 128))
def test_varlen_batch_invariance(gpu, d, causal, dtype):
    """A sequence's rows do not depend on its place in the batch: bitwise equal to a batch that
    holds it alone (same max_seqlen) and to the sequences packed in reverse order."""
    from exploring_flash_attention_amd import ops
    H, Hkv = 4, 2
    q, k, v, cu, lens = _batch(d, H, Hkv, dtype, seed=4)
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    full = ops.attention_varlen(qd, kd, vd, _cu_dev(cu, gpu), 257, causal=causal)
    for j, n in enumerate(lens):
        if n == 0:
            continue
        s = int(cu[j])
        alone = ops.attention_varlen(qd[s:s + n], kd[s:s + n], vd[s:s + n], _cu_dev([0, n], gpu), 257, causal=causal)
        assert torch.equal(alone, full[s:s + n]), (j, n)
    order = list(range(len(lens)))[::-1]
    rows = torch.cat([torch.arange(int(cu[j]), int(cu[j]) + lens[j]) for j in order])
    cu_r = np.concatenate([[0], np.cumsum([lens[j] for j in order])])
    rev = ops.attention_varlen(qd[rows.to(gpu)], kd[rows.to(gpu)], vd[rows.to(gpu)], _cu_dev(cu_r, gpu), 257,
                               causal=causal)
    assert torch.equal(rev, full[rows.to(gpu)])


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_reads_a_fused_qkv_projection_in_place(gpu, causal, monkeypatch):
    """q, k, v as slices of one [T, (H + 2 H_kv) d] tensor and out as a strided view: bitwise the
    contiguous call's result, one varlen kernel, the views' own pointers handed to the library
    and no device memory allocated by the call."""
    from exploring_flash_attention_amd import ops
    dtype, d, H, Hkv = torch.bfloat16, 128, 4, 2
    q, k, v, cu, lens = _batch(d, H, Hkv, dtype, seed=5)
    T = q.shape[0]
    cud = _cu_dev(cu, gpu)
    want = _sentinel_out(q, gpu)
    ops.attention_varlen(q.to(gpu), k.to(gpu), v.to(gpu), cud, 257, causal=causal, out=want)
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1).to(gpu)
    heads = qkv.view(T, H + 2 * Hkv, d)
    qv, kv, vv = heads[:, :H], heads[:, H:H + Hkv], heads[:, H + Hkv:]
    outbuf = torch.full((T, H, 2 * d), SENTINEL, dtype=dtype, device=gpu)
    outv = outbuf[..., :d]
    assert not (qv.is_contiguous() or kv.is_contiguous() or vv.is_contiguous() or outv.is_contiguous())
    handle = L.lib()
    real, seen = handle.fa_fwd_varlen, []

    def spy(*a):
        seen.append([x.value if isinstance(x, ctypes.c_void_p) else x for x in a[:5]])
        return real(*a)

    monkeypatch.setattr(handle, "fa_fwd_varlen", spy)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with ops.launched_kernels() as kl:
        assert ops.attention_varlen(qv, kv, vv, cud, 257, causal=causal, out=outv) is outv
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before, "the call allocated device memory (a copy?)"
    assert len(kl) == 1 and kl[0].startswith("fa_fwd_kernel<final, varlen") and "gqa" in kl[0], kl
    assert seen == [[qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), outv.data_ptr(), cud.data_ptr()]]
    assert torch.equal(outv, want)
    assert (outbuf[..., d:] == SENTINEL).all()  # the columns between the view's rows are untouched
    # poisoned sources after the call has finished: the result stands, and a second call on the
    # same views now reads the poison -- the views themselves are what the kernel reads
    qkv.fill_(float("nan"))
    assert torch.equal(outv, want)
    ops.attention_varlen(qv, kv, vv, cud, 257, causal=causal, out=outv)
    own = torch.from_numpy(_ref(d, H, Hkv, dtype, causal, 257, 5)[1].copy())
    assert torch.isnan(outv.cpu()[own].float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_varlen_corrupt_cu_seqlens_is_clamped(gpu, name):
    """A corrupt cu_seqlens on otherwise valid inputs: the call returns, the rows the clamped
    (start, len) name are finite, every other row of out and the guard rows behind it keep the
    sentinel.  (The clamp's address arithmetic is shown by the CPU replay above; q, k, v and out
    here are views of larger buffers all the same.)"""
    from exploring_flash_attention_amd import ops
    dtype, d, H, Hkv, T = torch.bfloat16, 128, 4, 2, 450
    g = torch.Generator().manual_seed(6)
    qb = torch.randn(T + GUARD, H, d, generator=g).to(dtype).to(gpu)
    kb, vb = (torch.randn(T + GUARD, Hkv, d, generator=g).to(dtype).to(gpu) for _ in range(2))
    cu = np.asarray(CORRUPT[name], np.int64)
    for causal, msl in ((False, 257), (True, 10000)):
        outb = torch.full((T + GUARD, H, d), SENTINEL, dtype=dtype, device=gpu)
        ops.attention_varlen(qb[:T], kb[:T], vb[:T], _cu_dev(cu, gpu), msl, causal=causal, out=outb[:T])
        torch.cuda.synchronize()
        st = np.clip(cu[:-1], 0, T)
        n = np.clip(cu[1:] - st, 0, np.minimum(T - st, min(msl, T)))
        owned = np.zeros(T + GUARD, bool)
        for s_, n_ in zip(st, n):
            owned[s_:s_ + n_] = True
        o = outb.cpu().float()
        own = torch.from_numpy(owned)
        assert torch.isfinite(o).all()
        assert (o[~own] == SENTINEL).all() and (o[own] != SENTINEL).all(), (name, causal)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_padded_head_dim(gpu, causal, dtype):
    """d = 80 has no kernel: zero-padded to 128 with the scale of d = 80."""
    from exploring_flash_attention_amd import ops
    lens = (1, 65, 0, 130)
    q, k, v, cu, _ = _batch(80, 4, 2, dtype, 7, lens)
    ref, owned = _ref(80, 4, 2, dtype, causal, 130, 7, lens)
    with ops.launched_kernels() as kl:
        o = ops.attention_varlen(q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu, gpu), 130, causal=causal)
    assert tuple(o.shape) == tuple(q.shape) and len(kl) == 1 and "varlen" in kl[0]
    _gate(o[torch.from_numpy(owned.copy())], ref[owned], dtype, f"padded d=80 causal={causal}")
    # out= keeps the rows of no sequence here too
    out = _sentinel_out(q, gpu)
    ops.attention_varlen(q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu, gpu), 130, causal=causal, out=out)
    assert torch.equal(out[torch.from_numpy(owned.copy())], o[torch.from_numpy(owned.copy())])
    assert (out.cpu()[torch.from_numpy(~owned)].float() == SENTINEL).all()


@pytest.mark.gpu
def test_varlen_empty_inputs_and_restrictions(gpu):
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    cu = _cu_dev([0, 0], gpu)
    e, ekv = torch.empty(0, 4, 64, dtype=bf, device=gpu), torch.empty(0, 2, 64, dtype=bf, device=gpu)
    with ops.launched_kernels() as kl:
        assert tuple(ops.attention_varlen(e, ekv, ekv, cu, 64).shape) == (0, 4, 64)
        q, kv = torch.zeros(8, 4, 64, dtype=bf, device=gpu), torch.zeros(8, 2, 64, dtype=bf, device=gpu)
        out = _sentinel_out(q, gpu)
        ops.attention_varlen(q, kv, kv, _cu_dev([0], gpu), 64, out=out)  # B = 0
        assert (out == SENTINEL).all()
    assert kl == []
    w = torch.zeros(8, 1, 384, dtype=bf, device=gpu)
    with pytest.raises(NotImplementedError, match="256"):
        ops.attention_varlen(w, w, w, _cu_dev([0, 8], gpu), 8)
    f = torch.zeros(8, 1, 64, dtype=torch.float64, device=gpu)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.attention_varlen(f, f, f, _cu_dev([0, 8], gpu), 8)
    with pytest.raises(ValueError, match="cu_seqlens"):
        ops.attention_varlen(q, kv, kv, torch.tensor([0, 8], dtype=torch.int32), 8)  # a host cu_seqlens
