"""Paged KV-cache decode: ops.attention_decode_paged / fa_fwd_decode_paged.

The decode forward of test_decode.py on a cache kept in pages of a shared pool: key j of batch b,
K/V head hkv lives in block block_table[b, j // page_size], row j % page_size of a
[num_blocks, page_size, H_kv, d] pool (csrc/fa_decode.hip, PAGED instantiations).

CPU: exports, the C entry's argument checks, Python refusals, and an address replay: a model of
the kernel's addressing rule restated in this file (as test_decode.py's replay is), walked over
every work item, tile and per-key causal access under a shuffled table.  The model is kept in
step with the library only where it can be on a CPU: every replayed geometry is first put to
fa_fwd_decode_paged's own argument checks (what the entry refuses is never replayed, and the
bounds the model relies on -- whole tiles per page, a table row that covers Lk -- are the ones the
entry enforces).  It does not run the kernel; the gate for the kernel is on the GPU: the outputs
are BITWISE those of attention_decode on the cache gathered in table order (same tiles, same
order, same arithmetic; only the addresses differ), hence inside test_decode.py's fp64 gate with
its values unchanged; plus the properties of what is and is not read.
"""
import ctypes
import functools
import itertools
import subprocess

import numpy as np
import pytest
import torch

import exploring_flash_attention_amd._lib as L
from test_decode import DTYPES, FAKE, GATE, HEADS, IDS, NULL, REPLAY, TILE, _bits, _gate, _sl, decode_ref

PAGES = (64, 128, 192)
LK = 1041  # max_seqlen_k of the GPU grid: no multiple of any page size, 17 tiles


# ----------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------


def test_paged_entry_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "fa_fwd_decode_paged" in names and "fa_fwd_decode_paged" in L.SIGNATURES
    assert len(L.SIGNATURES["fa_fwd_decode_paged"][1]) == 23
    assert L.lib().fa_version() == 0x000400  # an addition only


def test_paged_entry_argument_checks():
    lib = L.lib()
    BF = L.FA_DTYPE_BF16
    BIG = 1 << 30  # "enough" workspace bytes: nothing is launched before a check fails

    def err():
        return lib.fa_last_error()

    def call(q=FAKE, k=FAKE, v=FAKE, o=FAKE, bt=FAKE, sl=NULL, B=1, H=4, Hkv=2, Lq=1, Lk=640, d=128, nb=16, ps=128,
             ts=5, st=None, scale=0.1, flags=0, ns=2, ws=FAKE, wsb=BIG, dt=BF):
        return lib.fa_fwd_decode_paged(q, k, v, o, bt, sl, B, H, Hkv, Lq, Lk, d, nb, ps, ts, st, scale, flags, ns,
                                       ws, wsb, dt, NULL)

    INV, UNS = L.FA_ERR_INVALID_ARG, L.FA_ERR_UNSUPPORTED
    # the block table: required, 4-byte aligned
    assert call(bt=NULL) == INV and b"block_table" in err()
    assert call(bt=ctypes.c_void_p(0x10002)) == INV and b"block_table" in err()
    for bad in (0, -3):
        assert call(nb=bad) == INV and b"num_blocks" in err()
        assert call(ps=bad) == INV and b"page_size" in err()
    # table_stride >= ceil(Lk / page_size): 640 keys are 5 pages of 128, 641 are 6
    assert call(ts=4) == INV and b"table_stride" in err()
    assert call(Lk=641, ts=5) == INV and b"table_stride" in err()
    assert call(ts=0) == INV and b"table_stride" in err()
    # pool strides {block, head, row}: positive multiples of 8, rows at least d apart
    for bad in ((0, 128, 256), (32768, 4, 256), (32768, 128, 64), (-8, 128, 256)):
        assert call(st=(ctypes.c_int64 * 3)(*bad)) == INV and b"cache_strides" in err(), bad
    # no kernel: pages that are no whole tiles, a row stride past the descriptor's reach
    for ps in (16, 32, 96, 65, 200):
        assert call(ps=ps, ts=64) == UNS and b"page_size" in err() and b"multiple" in err(), ps
    assert call(ps=1 << 31, ts=64) == UNS and b"page_size" in err() and b"2^30" in err()
    assert call(st=(ctypes.c_int64 * 3)(1 << 28, 128, (1 << 20) + 8)) == UNS and b"stride" in err()
    # fa_fwd_decode's checks come first, unchanged
    for name in ("q", "k", "v", "o"):
        assert call(**{name: NULL}) == INV and b"null" in err()
        assert call(**{name: ctypes.c_void_p(0x10002)}) == INV and b"aligned" in err()
    assert call(sl=ctypes.c_void_p(0x10002)) == INV and b"seqlens_k" in err()
    for name in ("B", "H", "Lq", "Lk", "d"):
        assert call(**{name: 0}) == INV and b"positive" in err(), name
    for hkv in (0, 8, 3):
        assert call(Hkv=hkv) == INV and b"H_kv" in err()
    for bad in (0.0, -1.0, float("nan")):
        assert call(scale=bad) == INV and b"softmax_scale" in err()
    assert call(flags=2) == INV and b"flags" in err()
    assert call(ns=-1) == INV and b"num_splits" in err()
    assert call(ws=NULL) == INV and b"workspace" in err()
    assert call(wsb=16) == INV and b"workspace" in err()
    for d in (32, 96, 256):
        assert call(d=d) == UNS and str(d).encode() in err()
    assert call(H=8, Hkv=1, Lq=9) == UNS and b"Lq" in err()
    assert call(dt=L.FA_DTYPE_FP64) == UNS and b"FP64" in err()


def test_paged_python_refusals(monkeypatch):
    import exploring_flash_attention_amd as fa
    from exploring_flash_attention_amd import ops
    assert fa.attention_decode_paged is ops.attention_decode_paged and "attention_decode_paged" in fa.__all__
    assert "attention_decode_paged" in fa.__doc__
    bf = torch.bfloat16
    q = torch.zeros(2, 4, 1, 128, dtype=bf)
    pool = torch.zeros(8, 64, 2, 128, dtype=bf)
    bt = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):  # host tensors: refused as everywhere
        ops.attention_decode_paged(q, pool, pool, bt)
    # the checks behind the device check, on host tensors (nothing is launched before they raise)
    monkeypatch.setattr(ops, "_check_tensor", lambda *a, **k: None)
    for ps in (16, 96):
        p = torch.zeros(8, ps, 2, 128, dtype=bf)
        with pytest.raises(NotImplementedError, match=f"page_size={ps}"):
            ops.attention_decode_paged(q, p, p, bt)
    p80 = torch.zeros(8, 64, 2, 80, dtype=bf)
    with pytest.raises(NotImplementedError, match="d=80"):
        ops.attention_decode_paged(torch.zeros(2, 4, 1, 80, dtype=bf), p80, p80, bt)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.attention_decode_paged(q.double(), pool.double(), pool.double(), bt)
    with pytest.raises(NotImplementedError, match="attention_v1"):  # R = 2 * 33
        ops.attention_decode_paged(torch.zeros(2, 4, 33, 128, dtype=bf), pool, pool, bt)
    # views the kernel cannot address are refused, never copied: k / v strided differently, d not
    # contiguous, strides that are no multiples of 8
    other = torch.zeros(8, 2, 64, 128, dtype=bf).transpose(1, 2)
    with pytest.raises(NotImplementedError, match="strides"):
        ops.attention_decode_paged(q, pool, other, bt)
    with pytest.raises(NotImplementedError, match="strides"):
        t = torch.zeros(8, 64, 128, 2, dtype=bf).transpose(2, 3)
        ops.attention_decode_paged(q, t, t, bt)
    with pytest.raises(NotImplementedError, match="strides"):
        t = torch.zeros(8, 64, 2, 132, dtype=bf)[..., :128]
        ops.attention_decode_paged(q, t, t, bt)
    # the table: int32 [B, P]
    for bad in (bt.long(), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                torch.zeros(2, 6, dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="block_table"):
            ops.attention_decode_paged(q, pool, pool, bad)
    with pytest.raises(ValueError, match="max_seqlen_k=193 exceeds"):  # 3 pages of 64 keys map 192
        ops.attention_decode_paged(q, pool, pool, bt, max_seqlen_k=193)
    with pytest.raises(ValueError, match="max_seqlen_k=-1 must not be negative"):
        ops.attention_decode_paged(q, pool, pool, bt, max_seqlen_k=-1)
    with pytest.raises(ValueError, match="same shape"):
        ops.attention_decode_paged(q, pool, pool[:4], bt)
    with pytest.raises(ValueError, match="multiple"):
        p3 = torch.zeros(8, 64, 3, 128, dtype=bf)
        ops.attention_decode_paged(q, p3, p3, bt)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="seqlens_k"):
            ops.attention_decode_paged(q, pool, pool, bt, seqlens_k=bad)


# ---- address replay: a model of the addressing rule of the PAGED instantiations of csrc/fa_decode.hip


def entry_accepts(B, H, Hkv, Lq, Lk, d, ns, ps, nblk, ts, st):
    """fa_fwd_decode_paged's verdict on the geometry alone: every pointer fake and valid, the
    workspace pointer NULL, so that an accepted geometry stops at the workspace check (the last one
    before the launch) when the plan has splits.  Returns (status, message)."""
    lib = L.lib()
    status = lib.fa_fwd_decode_paged(FAKE, FAKE, FAKE, FAKE, FAKE, NULL, B, H, Hkv, Lq, Lk, d, nblk, ps, ts,
                                     (ctypes.c_int64 * 3)(*st), 0.1, L.FA_FWD_CAUSAL, ns, NULL, 0, L.FA_DTYPE_BF16, NULL)
    return status, lib.fa_last_error()


def kernel_cell(b, hkv, j, table, ts, ps, nblk, st):
    """Element offset of key j's row as the kernel computes it: the sequence's table row, the
    page j / page_size, the entry clamped into the pool, the row j % page_size inside the block."""
    e = table[b * ts + j // ps]
    blk = min(max(e, 0), nblk - 1)
    return blk * st[0] + hkv * st[1] + (j % ps) * st[2]


def paged_replay(B, H, Hkv, Lq, Lk, d, ns, ps, layout, table, nblk, seqlens=None, causal=True, cell=kernel_cell,
                 truth=None):
    """Walk every work item of the plan as the kernel does -- the 64-key MFMA tiles (one lookup
    and one descriptor per tile) and the causal keys folded one at a time -- and check each byte
    range: inside the pool allocation, and the cells of the logical keys under `truth` (the table
    the caller meant; None: no such check).  table: flat list, row stride len(table) // B.
    Returns (tiles, per-key accesses, table indices read)."""
    from exploring_flash_attention_amd import ops
    splits, kps, _ = ops.decode_plan(B, H, Hkv, Lq, Lk, d, ns, cus=256)
    assert kps % TILE == 0 and ps % ops.DECODE_PAGE_MULTIPLE == 0 and ops.DECODE_PAGE_MULTIPLE == TILE
    shape = (nblk, ps, Hkv, d) if layout == "bshd" else (nblk, Hkv, ps, d)
    alloc = torch.empty(shape, dtype=torch.bfloat16, device="meta")
    view = alloc if layout == "bshd" else alloc.transpose(1, 2)
    assert tuple(view.shape) == (nblk, ps, Hkv, d) and view.stride(3) == 1
    st = (view.stride(0), view.stride(2), view.stride(1))  # {block, head, row}
    alloc_bytes = alloc.numel() * 2
    ts = len(table) // B
    # The entry takes this geometry (two forced splits: it stops at the missing workspace, the last
    # check before the launch) and refuses what the model relies on not happening: a page that is
    # not whole tiles, a table row shorter than ceil(Lk / page_size).
    if Lk > TILE:
        status, msg = entry_accepts(B, H, Hkv, Lq, Lk, d, 2, ps, nblk, ts, st)
        assert status == L.FA_ERR_INVALID_ARG and b"workspace" in msg, msg
    status, msg = entry_accepts(B, H, Hkv, Lq, Lk, d, 2, ps + TILE // 2, nblk, ts, st)
    assert status == L.FA_ERR_UNSUPPORTED and b"page_size" in msg, msg
    status, msg = entry_accepts(B, H, Hkv, Lq, Lk, d, 2, ps, nblk, -(-Lk // ps) - 1, st)
    assert status == L.FA_ERR_INVALID_ARG and b"table_stride" in msg, msg
    assert ts * ps >= Lk
    read = set()

    def lookup(b, hkv, j):
        read.add(b * ts + j // ps)
        return cell(b, hkv, j, table, ts, ps, nblk, st)

    def check(lo, rows, b, hkv, j0, what):
        hi = lo + (rows - 1) * st[2] + d
        assert 0 <= lo and hi * 2 <= alloc_bytes, (what + " outside the pool", b, hkv, j0)
        if truth is not None:
            for r in range(rows):  # row r of the range is key j0 + r: its block, its row
                want = truth[b * ts + (j0 + r) // ps] * st[0] + hkv * st[1] + ((j0 + r) % ps) * st[2]
                assert lo + r * st[2] == want, (what + " of another key", b, hkv, j0 + r)

    tiles = keys = 0
    for b, hkv, s in itertools.product(range(B), range(Hkv), range(splits)):
        n = Lk if seqlens is None else min(max(seqlens[b], 0), Lk)
        kv_begin, kv_end = s * kps, min(s * kps + kps, n)
        if kv_begin >= n:
            continue
        all_end = max(n - Lq + 1, 0) if causal else n
        mf_end = min(kv_end, all_end)
        for t in range(-(-(mf_end - kv_begin) // TILE) if mf_end > kv_begin else 0):
            j0 = kv_begin + t * TILE
            check(lookup(b, hkv, j0), min(TILE, mf_end - j0), b, hkv, j0, "K/V tile")
            tiles += 1
        if causal and Lq > 1:
            for j in range(max(kv_begin, all_end), kv_end):
                check(lookup(b, hkv, j), 1, b, hkv, j, "causal key")
                keys += 1
        # only the entries of pages that hold a key of this split below len_b were read
        for idx in read:
            if idx // ts == b:
                assert (idx % ts) * ps < n, ("table entry past the sequence read", b, idx % ts, n)
    return tiles, keys, read


def _perm_table(B, P, nblk, seed=0, ts=None):
    """A seeded random assignment of distinct pool blocks to the B * P pages, as a flat list of
    row stride ts (>= P; the columns past P hold -1)."""
    ts = P if ts is None else ts
    blocks = np.random.default_rng(seed).permutation(nblk)[:B * P].reshape(B, P)
    tab = np.full((B, ts), -1, np.int64)
    tab[:, :P] = blocks
    return [int(x) for x in tab.reshape(-1)]


@pytest.mark.parametrize("ps", PAGES)
@pytest.mark.parametrize("case", REPLAY, ids=lambda c: "B%d-H%d-Hkv%d-Lq%d-Lk%d-d%d-ns%s" % c)
def test_paged_address_replay(case, ps):
    B, H, Hkv, Lq, Lk, d, ns = case
    P = -(-Lk // ps)
    nblk = B * P + 7  # more blocks than the sequences use
    for layout, causal in itertools.product(("bshd", "bhsd"), (False, True)):
        table = _perm_table(B, P, nblk, seed=ps + Lk)
        tiles, keys, read = paged_replay(B, H, Hkv, Lq, Lk, d, ns, ps, layout, table, nblk, causal=causal, truth=table)
        full = max(Lk - Lq + 1, 0) if causal else Lk
        assert keys == (B * Hkv * (Lk - full) if Lq > 1 else 0)
        assert tiles >= B * Hkv * -(-full // TILE)  # (a split boundary may cut the causal keys' tile in two)
        assert read == set(range(B * P))
        # per-sequence lengths: only the pages below them are looked up; the rest of the table is poison
        lens = [Lk] + [min(ps + 1, Lk)] * (B - 1)
        poisoned = list(table)
        for b in range(B):
            for p in range(-(-lens[b] // ps), P):
                poisoned[b * P + p] = -1
        _, _, read = paged_replay(B, H, Hkv, Lq, Lk, d, ns, ps, layout, poisoned, nblk, seqlens=lens, causal=causal,
                                  truth=poisoned)
        assert all(poisoned[i] >= 0 for i in read)
    # a table wider than ceil(Lk / page_size)
    wide = _perm_table(B, P, nblk, seed=1, ts=P + 3)
    paged_replay(B, H, Hkv, Lq, Lk, d, ns, ps, "bshd", wide, nblk, truth=wide)


def test_paged_replay_shared_prefix():
    """Two sequences whose first pages are the same physical blocks."""
    B, H, Hkv, Lq, Lk, d, ps = 2, 4, 2, 3, 1041, 128, 128
    P = -(-Lk // ps)
    nblk = 2 * P
    table = _perm_table(B, P, nblk, seed=3)
    table[P:P + 3] = table[0:3]
    for layout in ("bshd", "bhsd"):
        paged_replay(B, H, Hkv, Lq, Lk, d, None, ps, layout, table, nblk, seqlens=[700, 3 * ps + 1], truth=table)


def test_paged_replay_catches_wrong_addressing():
    B, H, Hkv, Lq, Lk, d = 2, 4, 2, 3, 1041, 128
    mutations = {
        "the logical page as the physical block":
            lambda b, hkv, j, table, ts, ps, nblk, st: (j // ps) * st[0] + hkv * st[1] + (j % ps) * st[2],
        "the in-page row offset dropped":
            lambda b, hkv, j, table, ts, ps, nblk, st: table[b * ts + j // ps] * st[0] + hkv * st[1],
        "batch 0's table row for every batch":
            lambda b, hkv, j, table, ts, ps, nblk, st: table[j // ps] * st[0] + hkv * st[1] + (j % ps) * st[2],
        "j / 64 as the page index":
            lambda b, hkv, j, table, ts, ps, nblk, st: (table[min(b * ts + j // TILE, len(table) - 1)] * st[0]
                                                        + hkv * st[1] + (j % ps) * st[2]),
    }
    for ps, layout in itertools.product((128, 192), ("bshd", "bhsd")):
        P = -(-Lk // ps)
        nblk = B * P + 7
        table = _perm_table(B, P, nblk, seed=ps)
        for ns, causal in ((2, True), (None, False)):
            paged_replay(B, H, Hkv, Lq, Lk, d, ns, ps, layout, table, nblk, causal=causal, truth=table)
            for what, cell in mutations.items():
                with pytest.raises(AssertionError, match="K/V tile|causal key"):
                    paged_replay(B, H, Hkv, Lq, Lk, d, ns, ps, layout, table, nblk, causal=causal, cell=cell, truth=table)
    # the per-key causal keys alone straddle a page: len = page_size + 1 at Lq = 3 (keys ps - 1 and ps)
    ps, P = 128, 9
    table = _perm_table(B, P, B * P, seed=5)
    _, keys, _ = paged_replay(B, H, Hkv, Lq, Lk, d, 1, ps, "bshd", table, B * P, seqlens=[ps + 1, ps + 1], truth=table)
    assert keys == B * Hkv * 2
    with pytest.raises(AssertionError, match="causal key"):  # the first page kept for the key behind its end
        paged_replay(B, H, Hkv, Lq, Lk, d, 1, ps, "bshd", table, B * P, seqlens=[ps + 1, ps + 1], truth=table,
                     cell=lambda b, hkv, j, table, ts, ps, nblk, st:
                     table[b * ts + min(j, ps - 1) // ps] * st[0] + hkv * st[1] + (j % ps) * st[2])


def test_paged_replay_clamps_corrupt_entries():
    """Entries outside [0, num_blocks) are clamped before they enter an address: every range stays
    inside the pool (what it then reads is the wrong block -- a wrong answer, no stray access)."""
    B, H, Hkv, Lq, Lk, d, ps = 2, 4, 2, 3, 1041, 128, 192
    P = -(-Lk // ps)
    nblk = B * P + 2
    for layout in ("bshd", "bhsd"):
        st = (ps * Hkv * d, d, Hkv * d) if layout == "bshd" else (Hkv * ps * d, ps * d, d)
        for bad in (-1, nblk + 5, -(1 << 31), (1 << 31) - 1):
            table = _perm_table(B, P, nblk, seed=7)
            table[1], table[P + 2] = bad, bad
            paged_replay(B, H, Hkv, Lq, Lk, d, 2, ps, layout, table, nblk)
            assert kernel_cell(0, 0, ps, table, P, ps, nblk, st) == (0 if bad < 0 else nblk - 1) * st[0]
            with pytest.raises(AssertionError, match="outside the pool"):  # ... and without the clamp it would not
                paged_replay(B, H, Hkv, Lq, Lk, d, 2, ps, layout, table, nblk,
                             cell=lambda b, hkv, j, table, ts, ps, nblk, st:
                             table[b * ts + j // ps] * st[0] + hkv * st[1] + (j % ps) * st[2])


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=4)
def _pools(nblk, ps, Hkv, d, dtype, seed=0):
    """Seeded storage-rounded host pools K, V [nblk, ps, Hkv, d]; nobody writes to them."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(nblk, ps, Hkv, d, generator=g).to(dtype) for _ in range(2))


@functools.lru_cache(maxsize=None)
def _q(B, H, Lq, d, dtype, seed=0):
    return torch.randn(B, H, Lq, d, generator=torch.Generator().manual_seed(100 + seed)).to(dtype)


def _table(B, P, nblk, seed=0):
    return torch.tensor(_perm_table(B, P, nblk, seed), dtype=torch.int32).reshape(B, P)


def _gather(pool, table, Lk):
    """The contiguous cache [B, Hkv, Lk, d] a caller without paging has to build: the pages of
    every sequence in table order."""
    B, P = table.shape
    g = pool[table.reshape(-1).long().to(pool.device)]  # [B * P, ps, Hkv, d]
    return g.reshape(B, P * pool.shape[1], pool.shape[2], pool.shape[3]).transpose(1, 2)[:, :, :Lk].contiguous()


def _lens_sets(ps):
    """{0, 1, 63, 64, 65, ps - 1, ps, ps + 1, 2 ps + 37, 1041} mixed within batches of three."""
    return ((0, ps + 1, LK), (1, 63, 2 * ps + 37), (64, 65, ps), (ps - 1, ps + 1, 2000))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("ps", PAGES)
@pytest.mark.parametrize("d", (64, 128))
def test_paged_is_bitwise_the_contiguous_decode(gpu, d, ps, dtype):
    """The main gate: bit for bit attention_decode on the gathered cache, and with it inside the
    fp64 gate of test_decode.py; the kernel label."""
    from exploring_flash_attention_amd import ops
    B = 3
    P = -(-LK // ps)
    nblk = B * P + 5
    table = _table(B, P, nblk, seed=ps + d)
    td = table.to(gpu)
    worst = 0.0
    for H, Hkv in HEADS:
        kp, vp = (t.to(gpu) for t in _pools(nblk, ps, Hkv, d, dtype))
        kc, vc = _gather(kp, table, LK), _gather(vp, table, LK)
        kn, vn = kc.double().cpu().numpy(), vc.double().cpu().numpy()
        for Lq, causal, lens in itertools.product((1, 3, 8), (False, True), _lens_sets(ps)):
            qd = _q(B, H, Lq, d, dtype).to(gpu)
            sl = _sl(lens, gpu)
            ref = decode_ref(qd.double().cpu().numpy(), kn, vn, lens, causal)
            for ns in (None, 1, 2, 5):
                label = f"paged ps{ps} H{H}/{Hkv} Lq{Lq} d{d} {IDS[dtype]} causal={causal} lens={lens} ns={ns}"
                want = ops.attention_decode(qd, kc, vc, seqlens_k=sl, causal=causal, num_splits=ns)
                with ops.launched_kernels() as kl:
                    got = ops.attention_decode_paged(qd, kp, vp, td, seqlens_k=sl, max_seqlen_k=LK, causal=causal,
                                                     num_splits=ns)
                assert got.dtype == dtype and tuple(got.shape) == (B, H, Lq, d)
                assert torch.equal(_bits(got), _bits(want)), label
                splits = ops.decode_plan(B, H, Hkv, Lq, LK, d, ns, dtype)[0]
                assert len(kl) == 1 and kl[0].startswith("fa_decode_kernel<") and ", paged>" in kl[0], kl
                assert f"[grid {B * Hkv * splits}]" in kl[0].split(" + ")[0], (kl, splits)
                assert ("fa_decode_combine_kernel" in kl[0]) == (splits > 1), kl
                worst = max(worst, _gate(got, ref, dtype, label, quiet=True))
            assert (_bits(got[0]) == 0).all() or lens[0] > 0
    print(f"worst err/bound over heads, Lq, lengths, splits: {worst:.3f}")


def _poisoned(pool, table, lens, ps, fill):
    """pool with everything no sequence's first len_b keys occupy replaced by fill: unused blocks,
    the rows of a last page at or past len_b, whole pages past len_b that the table still maps."""
    out = torch.full_like(pool, fill)
    for b, n in enumerate(lens):
        for p in range(-(-n // ps)):
            rows = min(ps, n - p * ps)
            out[table[b, p], :rows] = pool[table[b, p], :rows]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_paged_reads_nothing_past_the_lengths(gpu, d, dtype):
    from exploring_flash_attention_amd import ops
    B, H, Hkv, Lq = 3, 4, 2, 3
    huge = torch.finfo(dtype).max  # the dtype's largest finite value
    for ps in (64, 192):
        P = -(-LK // ps)
        nblk = B * P + 5
        lens = (2 * ps + 37, ps + 1, 0)
        table = _table(B, P, nblk, seed=11)
        kp, vp = _pools(nblk, ps, Hkv, d, dtype)
        qd, sl = _q(B, H, Lq, d, dtype).to(gpu), _sl(lens, gpu)
        for ns, causal in itertools.product((None, 1, 5), (False, True)):
            clean = ops.attention_decode_paged(qd, kp.to(gpu), vp.to(gpu), table.to(gpu), seqlens_k=sl, max_seqlen_k=LK,
                                               causal=causal, num_splits=ns)
            assert torch.isfinite(clean.float()).all()
            for fill, entry in itertools.product((float("nan"), huge), (-1, 2 ** 31 - 1)):
                tb = table.clone()
                for b, n in enumerate(lens):
                    tb[b, -(-n // ps):] = entry
                o = ops.attention_decode_paged(qd, _poisoned(kp, table, lens, ps, fill).to(gpu),
                                               _poisoned(vp, table, lens, ps, fill).to(gpu), tb.to(gpu), seqlens_k=sl,
                                               max_seqlen_k=LK, causal=causal, num_splits=ns)
                assert torch.equal(_bits(o), _bits(clean)), (ps, ns, causal, fill, entry)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_paged_causal_mask_across_a_page_boundary(gpu, d, dtype):
    """NaN in V at the keys a causal row may not see leaves that row bitwise unchanged, also when
    those keys sit in the next page; the last row does see them."""
    from exploring_flash_attention_amd import ops
    B, H, Hkv, Lq, ps = 2, 4, 2, 3, 128
    P = -(-LK // ps)
    nblk = B * P + 5
    table = _table(B, P, nblk, seed=13)
    kp, vp = _pools(nblk, ps, Hkv, d, dtype)
    qd = _q(B, H, Lq, d, dtype).to(gpu)
    for ns, lens in itertools.product((None, 1, 3), ((ps + 1, 150), (ps + 2, 2 * ps), (LK, 37))):
        sl = _sl(lens, gpu)
        clean = ops.attention_decode_paged(qd, kp.to(gpu), vp.to(gpu), table.to(gpu), seqlens_k=sl, max_seqlen_k=LK,
                                           num_splits=ns)
        for i in range(Lq - 1):
            vg = vp.clone()
            for b, n in enumerate(lens):
                for j in range(n - (Lq - 1 - i), n):
                    vg[table[b, j // ps], j % ps] = float("nan")
            o = ops.attention_decode_paged(qd, kp.to(gpu), vg.to(gpu), table.to(gpu), seqlens_k=sl, max_seqlen_k=LK,
                                           num_splits=ns)
            assert torch.equal(_bits(o[:, :, :i + 1]), _bits(clean[:, :, :i + 1])), ("NaN V behind the mask", ns, lens, i)
            assert torch.isnan(o[:, :, Lq - 1].float()).all()  # the last row does see them


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_paged_pool_layouts_and_table_views(gpu, d, dtype):
    from exploring_flash_attention_amd import ops
    B, H, Hkv, Lq, ps = 3, 4, 2, 3, 192
    P = -(-LK // ps)
    nblk = B * P + 5
    table = _table(B, P, nblk, seed=17)
    kp, vp = (t.to(gpu) for t in _pools(nblk, ps, Hkv, d, dtype))
    # the same pool stored [num_blocks, H_kv, page_size, d], passed transposed
    kt, vt = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (kp, vp))
    assert kt.stride() == (Hkv * ps * d, d, ps * d, 1) and not kt.is_contiguous()
    # the table as a column slice of a wider tensor
    wide = torch.full((B, P + 5), -7, dtype=torch.int32, device=gpu)
    wide[:, 2:2 + P] = table.to(gpu)
    tv = wide[:, 2:2 + P]
    assert tv.stride() == (P + 5, 1) and not tv.is_contiguous()
    qd, sl = _q(B, H, Lq, d, dtype).to(gpu), _sl((LK, ps + 1, 500), gpu)
    for ns, causal in itertools.product((None, 2), (False, True)):
        a = ops.attention_decode_paged(qd, kp, vp, table.to(gpu), seqlens_k=sl, max_seqlen_k=LK, causal=causal, num_splits=ns)
        with ops.launched_kernels() as kl:
            b = ops.attention_decode_paged(qd, kt, vt, table.to(gpu), seqlens_k=sl, max_seqlen_k=LK, causal=causal,
                                           num_splits=ns)
        assert len(kl) == 1 and kl[0].count("fa_decode_kernel<") == 1, kl  # read in place: nothing else ran
        c = ops.attention_decode_paged(qd, kp, vp, tv, seqlens_k=sl, max_seqlen_k=LK, causal=causal, num_splits=ns)
        assert torch.equal(_bits(a), _bits(b)), ("transposed pool", ns, causal)
        assert torch.equal(_bits(a), _bits(c)), ("table view", ns, causal)
    ref = decode_ref(qd.double().cpu().numpy(), _gather(kp, table, LK).double().cpu().numpy(),
                     _gather(vp, table, LK).double().cpu().numpy(), (LK, ps + 1, 500), True)
    _gate(b, ref, dtype, "transposed pool")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_paged_shared_prefix(gpu, dtype):
    from exploring_flash_attention_amd import ops
    B, H, Hkv, Lq, d, ps = 2, 8, 1, 3, 128, 128
    P = -(-LK // ps)
    nblk = B * P
    table = _table(B, P, nblk, seed=19)
    table[1, :3] = table[0, :3]  # the first 384 keys of both sequences are the same blocks
    kp, vp = (t.to(gpu) for t in _pools(nblk, ps, Hkv, d, dtype))
    kc, vc = _gather(kp, table, LK), _gather(vp, table, LK)
    assert torch.equal(kc[0, :, :3 * ps], kc[1, :, :3 * ps]) and not torch.equal(kc[0, :, 3 * ps:], kc[1, :, 3 * ps:])
    qd = _q(B, H, Lq, d, dtype).to(gpu)
    for ns, lens in itertools.product((None, 1), ((700, 3 * ps + 1), (300, 384))):
        sl = _sl(lens, gpu)
        got = ops.attention_decode_paged(qd, kp, vp, table.to(gpu), seqlens_k=sl, max_seqlen_k=LK, num_splits=ns)
        want = ops.attention_decode(qd, kc, vc, seqlens_k=sl, num_splits=ns)
        assert torch.equal(_bits(got), _bits(want)), (ns, lens)
        _gate(got, decode_ref(qd.double().cpu().numpy(), kc.double().cpu().numpy(), vc.double().cpu().numpy(), lens, True),
              dtype, f"shared prefix ns={ns} lens={lens}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_paged_max_seqlen_k(gpu, dtype):
    from exploring_flash_attention_amd import ops
    B, H, Hkv, Lq, d, ps, Lmax = 2, 4, 2, 3, 128, 128, 300
    P = -(-Lmax // ps)  # 3 pages
    nblk = B * P + 4
    table = _table(B, P, nblk, seed=23)
    kp, vp = (t.to(gpu) for t in _pools(nblk, ps, Hkv, d, dtype))
    kc, vc = _gather(kp, table, Lmax), _gather(vp, table, Lmax)
    qd = _q(B, H, Lq, d, dtype).to(gpu)
    # a table with more columns than ceil(max_seqlen_k / page_size), garbage in them
    wide = torch.cat([table, torch.tensor([[-1, 2 ** 31 - 1, nblk + 9]] * B, dtype=torch.int32)], dim=1).to(gpu)
    for ns, causal in itertools.product((None, 1, 2), (False, True)):
        want = ops.attention_decode(qd, kc, vc, causal=causal, num_splits=ns)
        # lengths above max_seqlen_k are clamped to it; None means max_seqlen_k
        for sl in (None, _sl((5000, Lmax), gpu)):
            a = ops.attention_decode_paged(qd, kp, vp, table.to(gpu), seqlens_k=sl, max_seqlen_k=Lmax, causal=causal,
                                           num_splits=ns)
            assert torch.equal(_bits(a), _bits(want)), (ns, causal, sl)
        with ops.launched_kernels() as kl:
            b = ops.attention_decode_paged(qd, kp, vp, wide, seqlens_k=_sl((Lmax, Lmax), gpu), max_seqlen_k=Lmax,
                                           causal=causal, num_splits=ns)
        assert torch.equal(_bits(b), _bits(want)), ("wide table", ns, causal)
        # the plan is the one for max_seqlen_k, not for the table's width
        splits = ops.decode_plan(B, H, Hkv, Lq, Lmax, d, ns, dtype)[0]
        assert f"[grid {B * Hkv * splits}]" in kl[0].split(" + ")[0], (kl, splits)
    # max_seqlen_k = None: all the table maps (here 3 pages = 384 keys), lengths bound what is read
    c = ops.attention_decode_paged(qd, kp, vp, table.to(gpu), seqlens_k=_sl((Lmax, 77), gpu))
    want = ops.attention_decode(qd, _gather(kp, table, P * ps), _gather(vp, table, P * ps), seqlens_k=_sl((Lmax, 77), gpu))
    assert torch.equal(_bits(c), _bits(want))


@pytest.mark.gpu
def test_paged_workspace_reuse_and_out(gpu):
    from exploring_flash_attention_amd import ops
    dtype = torch.bfloat16
    B, H, Hkv, Lq, d, ps = 2, 4, 2, 3, 128, 192
    P = -(-LK // ps)
    nblk = B * P + 5
    table = _table(B, P, nblk, seed=29).to(gpu)
    kp, vp = (t.to(gpu) for t in _pools(nblk, ps, Hkv, d, dtype))
    qd = _q(B, H, Lq, d, dtype).to(gpu)
    splits, _, nbytes = ops.decode_plan(B, H, Hkv, Lq, LK, d, 5, dtype)
    assert splits == 5 and nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)  # never reset by the caller
    out = torch.full((B, H, Lq, d), float("nan"), dtype=dtype, device=gpu)
    firsts = {}
    for lens in ((37, LK), (LK, 500), (37, LK)):  # different lengths through one workspace, no reset
        sl = _sl(lens, gpu)
        a = ops.attention_decode_paged(qd, kp, vp, table, seqlens_k=sl, max_seqlen_k=LK, num_splits=5, workspace=ws, out=out)
        assert a is out
        first = _bits(a).clone()
        b = ops.attention_decode_paged(qd, kp, vp, table, seqlens_k=sl, max_seqlen_k=LK, num_splits=5, workspace=ws, out=out)
        assert torch.equal(first, _bits(b))
        c = ops.attention_decode_paged(qd, kp, vp, table, seqlens_k=sl, max_seqlen_k=LK, num_splits=5)
        assert torch.equal(first, _bits(c))
        assert torch.equal(firsts.setdefault(lens, first), first)
    with pytest.raises(ValueError, match="workspace too small"):
        ops.attention_decode_paged(qd, kp, vp, table, max_seqlen_k=LK, num_splits=5, workspace=ws[:nbytes - 1])
    # empty inputs: no launch
    with ops.launched_kernels() as kl:
        e = ops.attention_decode_paged(qd[:0], kp, vp, table[:0])
        z = ops.attention_decode_paged(qd, kp, vp, table[:, :0])
    assert kl == [] and e.numel() == 0 and tuple(z.shape) == (B, H, Lq, d) and (z == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_paged_wide_row_tiles(gpu, d, dtype):
    """G * Lq = 64: the 64-row instantiation (H32 H_kv8 Lq 8, causal), and the 32-row one."""
    from exploring_flash_attention_amd import ops
    B, Lk, ps = 2, 300, 128
    P = -(-Lk // ps)
    nblk = B * P + 3
    table = _table(B, P, nblk, seed=31)
    for (H, Hkv, Lq), ns in itertools.product(((32, 8, 8), (8, 2, 8)), (None, 3)):
        kp, vp = (t.to(gpu) for t in _pools(nblk, ps, Hkv, d, dtype))
        kc, vc = _gather(kp, table, Lk), _gather(vp, table, Lk)
        qd = _q(B, H, Lq, d, dtype).to(gpu)
        for lens in (None, (Lk, ps + 1), (130, 5)):
            with ops.launched_kernels() as kl:
                got = ops.attention_decode_paged(qd, kp, vp, table.to(gpu), seqlens_k=_sl(lens, gpu), max_seqlen_k=Lk,
                                                 num_splits=ns)
            R = H // Hkv * Lq
            assert f"<{32 if R <= 32 else 64} rows, paged>" in kl[0], kl
            want = ops.attention_decode(qd, kc, vc, seqlens_k=_sl(lens, gpu), num_splits=ns)
            assert torch.equal(_bits(got), _bits(want)), (H, Hkv, Lq, ns, lens)
            _gate(got, decode_ref(qd.double().cpu().numpy(), kc.double().cpu().numpy(), vc.double().cpu().numpy(), lens, True),
                  dtype, f"paged R={R} d{d} ns={ns} lens={lens}", quiet=True)


@pytest.mark.gpu
def test_paged_clamps_corrupt_entries_on_the_device(gpu):
    """A used entry outside [0, num_blocks) reads the clamped block: the result is the one of the
    table with 0 / num_blocks - 1 in its place.  (The pool is a slice of a larger tensor.)"""
    from exploring_flash_attention_amd import ops
    dtype = torch.bfloat16
    B, H, Hkv, Lq, d, ps, Lk = 2, 4, 2, 3, 128, 64, 300
    P = -(-Lk // ps)
    nblk = B * P + 3
    table = _table(B, P, nblk, seed=37)
    kp, vp = _pools(nblk, ps, Hkv, d, dtype)
    big_k, big_v = (torch.zeros((nblk + 16, ps, Hkv, d), dtype=dtype, device=gpu) for _ in range(2))
    big_k[8:8 + nblk], big_v[8:8 + nblk] = kp.to(gpu), vp.to(gpu)
    kd, vd = big_k[8:8 + nblk], big_v[8:8 + nblk]
    qd = _q(B, H, Lq, d, dtype).to(gpu)
    for bad, to in ((-1, 0), (nblk + 5, nblk - 1)):
        corrupt, fixed = table.clone(), table.clone()
        corrupt[0, 1], corrupt[1, P - 1] = bad, bad
        fixed[0, 1], fixed[1, P - 1] = to, to
        for ns in (None, 1):
            a = ops.attention_decode_paged(qd, kd, vd, corrupt.to(gpu), max_seqlen_k=Lk, num_splits=ns)
            b = ops.attention_decode_paged(qd, kd, vd, fixed.to(gpu), max_seqlen_k=Lk, num_splits=ns)
            assert torch.equal(_bits(a), _bits(b)), (bad, ns)
