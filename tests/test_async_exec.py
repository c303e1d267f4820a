"""The execution side of the operators: stream order, two streams at once, graph capture and
replay, and the tensor's device against the current one.

Every comparison is BITWISE against the same call made eagerly on the default stream of cuda:0
with a full synchronise on both sides (the kernels are deterministic); no tolerance is added.
So that the baseline itself is known good, each eager result is gated once against the fp64
reference with the helpers and tolerances of the files that own them (test_gpu._ref / _gate,
test_gqa.gqa_ref / _gate, test_decode.decode_ref / _gate, test_varlen.varlen_ref / _gate, 1e-12 for the
fp64 kernels as test_gpu.test_fp64_paths).

One table, ROWS, serves every part.  A row owns the shapes, the seeded host data of its static
input buffers (data(seed): other seeds change the values AND the lengths, tables and offsets),
its scratch tensors (out, workspace), the call, and the kernel names the call must launch,
asserted through ops.launched_kernels() in the eager run.

Part 1  the caller's stream is the stream: inputs NaN (lengths, tables, offsets zero), then on a
        side stream a delay, the copies that put the real inputs in place, the call and a clone;
        only that stream is synchronised.  A launch, a counter reset, a second kernel or a torch
        temporary on any other stream reads the stale inputs.  The delay is DELAY_MS = 20 ms of
        torch.cuda._sleep (cycles from one timed spin; a chain of matmuls where _sleep is
        missing); it is not asserted on.  The control, the same harness with the call made on
        the default stream, must NOT match: on the MI355X it differed for every control row
        (NaN, or the zero rows of empty sequences, out), 0.1-0.3 ms into the 19.4 ms the side
        stream stayed busy, so 20 ms is long enough.  The side streams are chosen once so that
        they do not share a hardware queue with the default stream (_side_streams): on a shared
        queue the control matches and a misplaced launch would go unnoticed.
Part 2  two side streams, each with its own inputs, outputs and workspaces, eight rounds
        enqueued alternately without a synchronise.
Part 3  one call captured on one stream (a straight-line graph), replayed after the contents of
        the static tensors changed in place -- values, seqlens_k with a 0 and the full length,
        a reshuffled block table over a pool moved to match, a new cu_seqlens of the same total.
        Planted defect: a decode call that reads a clone of seqlens_k taken at capture time
        (a library that copied the lengths) must be rejected.
Part 4  tensors on cuda:1 while cuda:0 is current (skipped with one GPU).
"""
import ctypes
import functools
import time
import zlib

import numpy as np
import pytest
import torch

import exploring_flash_attention_amd._lib as L
import test_decode
import test_gqa
import test_varlen
from test_decode import decode_ref
from test_gpu import _gate as gate_mha
from test_gpu import _ref as ref_mha
from test_gqa import gqa_ref
from test_varlen import varlen_ref
from test_weight_readout import chain_cases

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
IDS = {BF: "bf16", HF: "fp16", torch.float64: "fp64"}
INT = {BF: torch.int16, HF: torch.int16, torch.float64: torch.int64}
DELAY_MS = 20
ROUNDS = 8
WAIT_S = 60  # a stream that has not finished by then is reported as hung


# ----------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------


class Row:
    """name; kernels: per library call the kernel names it must enqueue; data(seed) -> {buffer
    name: host tensor} (keys with a leading underscore are for check() only, not buffers);
    scratch(dev) -> {name: device tensor} (out*: result buffers, workspace); call(bufs, x) -> the
    result tensor; check(out_cpu, data): the fp64 gate; fresh_ws: the workspace is handed over
    with garbage in it (the library resets its counters itself).  The fp64 reference of the
    rows that fill the chip (HEAVY) takes seconds: their eager result is gated at seed 0 only."""

    def __init__(self, name, kernels, data, call, check, scratch=lambda dev: {}, fresh_ws=False):
        self.name, self.kernels, self.data, self.call, self.check = name, kernels, data, call, check
        self.scratch, self.fresh_ws = scratch, fresh_ws


HEAVY = ("v1-chain", "v1-chain-gqa", "v2-fused-walk", "v2-arrive-first")


ROWS = {}


def _row(*a, **kw):
    r = Row(*a, **kw)
    assert r.name not in ROWS
    ROWS[r.name] = r


def _gen(name, seed):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % (1 << 30) + seed)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ops():
    from exploring_flash_attention_amd import ops
    return ops


def _qkv(name, seed, B, H, Hkv, L_, d, dtype):
    g = _gen(name, seed)
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    q = torch.randn(B, H, L_, d, generator=g, dtype=wide).to(dtype)
    k, v = (torch.randn(B, Hkv, L_, d, generator=g, dtype=wide).to(dtype) for _ in range(2))
    return {"q": q, "k": k, "v": v}


def _check_mha(dtype):
    def check(out, x):
        if dtype == torch.float64:
            assert np.abs(out.numpy() - ref_mha(x["q"], x["k"], x["v"])).max() <= 1e-12
        else:
            gate_mha(out, ref_mha(x["q"], x["k"], x["v"]), dtype)
    return check


def _gqa(x, causal=False):
    return gqa_ref(*(x[n].double().numpy() for n in "qkv"), causal=causal)


def _v1_row(name, kernel, shape, dtype=BF, call=None, check=None, scratch=lambda dev: {}, data=None):
    """attention_v1 on q, k, v of `shape` = (B, H, Hkv, L, d), or a callable giving it (the chained
    rows size themselves from the device's compute units)."""
    dims = shape if callable(shape) else (lambda: shape)
    _row(name, [[kernel]], data or (lambda seed: _qkv(name, seed, *dims(), dtype)),
         call or (lambda b, x: _ops().attention_v1(b["q"], b["k"], b["v"])), check or _check_mha(dtype), scratch)


_v1_row("v1-tail-d64", "fa_fwd_kernel<final>", (2, 3, 3, 200, 64))
_v1_row("v1-16x16-d128", "fa_fwd16_kernel<final>", (1, 2, 2, 256, 128))
# one query tile per workgroup of the persistent grid (2 per CU): the smallest chained launch
_v1_row("v1-chain", "fa_fwd16_chain_kernel<final>", lambda: (1,) + chain_cases(_cus())["one-item"] + (128,))
_v1_row("v1-chain-gqa", "fa_fwd16_chain_kernel<final, gqa>", lambda: (1,) + chain_cases(_cus())["gqa"] + (128,),
        check=lambda out, x: test_gqa._gate(out, _gqa(x), BF, "v1-chain-gqa"))
_v1_row("v1-causal-gqa", "fa_fwd_kernel<final, causal, gqa>", (2, 4, 2, 200, 64),
        call=lambda b, x: _ops().attention_v1(b["q"], b["k"], b["v"], causal=True),
        check=lambda out, x: test_gqa._gate(out, _gqa(x, causal=True), BF, "v1-causal-gqa"))


def _blhd(seed):
    return {n: t.transpose(1, 2).contiguous() for n, t in _qkv("v1-strided", seed, 2, 3, 3, 200, 64, BF).items()}


# q, k, v live as [B, L, H, d]; the operator sees their [B, H, L, d] views and addresses them in place
_v1_row("v1-strided", "fa_fwd_kernel<final, strided>", None, data=_blhd,
        call=lambda b, x: _ops().attention_v1(*(b[n].transpose(1, 2) for n in "qkv")),
        check=lambda out, x: gate_mha(out, ref_mha(*(x[n].transpose(1, 2) for n in "qkv")), BF))
# d = 80 runs the d = 128 kernel on zero-padded copies and copies the first 80 columns back
_v1_row("v1-padded-d80", "fa_fwd_kernel<final>", (2, 2, 2, 130, 80))
# an out view whose row stride (68) the strided kernel cannot address: a contiguous result is
# computed and copied back into the view
_v1_row("v1-out-copy-back", "fa_fwd_kernel<final>", (2, 2, 2, 200, 64),
        call=lambda b, x: _ops().attention_v1(b["q"], b["k"], b["v"], out=x["out_buf"][..., :64]),
        scratch=lambda dev: {"out_buf": torch.empty(2, 2, 200, 68, dtype=BF, device=dev)})
_row("tiled-d512", [["fa_fwd_dt_kernel<paired>"]], lambda seed: _qkv("tiled-d512", seed, 1, 2, 2, 130, 512, BF),
     lambda b, x: _ops().attention_tiled_d(b["q"], b["k"], b["v"]), _check_mha(BF))


def _v2_row(name, kernels, shape, dtype, kw, fresh_ws=False, zeroed=False, plan=None):
    """attention_v2 with out and workspace given; plan: the (key blocks, blocks per workgroup,
    partials per tile) the shape must be scheduled as."""
    def dims():
        return shape() if callable(shape) else shape

    def scratch(dev):
        B, H, L_, d = dims()
        ops = _ops()
        with torch.cuda.device(dev):
            nbytes = ops.v2_workspace_bytes(B, H, L_, d, kw["kv_tiles_per_block"], dtype, kw.get("partial_dtype"),
                                            kw.get("blocks_per_workgroup"))[0]
        make = torch.zeros if zeroed else torch.empty
        return {"out": torch.empty(B, H, L_, d, dtype=dtype, device=dev),
                "workspace": make(nbytes, dtype=torch.uint8, device=dev)}

    def call(b, x):
        B, H, L_, d = dims()
        ops = _ops()
        if plan is not None:
            got = ops.v2_split_plan(B, H, L_, d, kw["kv_tiles_per_block"], dtype, kw.get("blocks_per_workgroup"))
            assert got == plan, (name, got)
        return ops.attention_v2(b["q"], b["k"], b["v"], out=x.get("out"), workspace=x.get("workspace"),
                                workspace_zeroed=zeroed and "workspace" in x, **kw)

    _row(name, [kernels], lambda seed: _qkv(name, seed, dims()[0], dims()[1], dims()[1], dims()[2], dims()[3], dtype),
         call, _check_mha(dtype), scratch, fresh_ws)


FUSED = "<fused split, in-kernel combine>"
for _dt in (BF, HF):
    # four partials of 128 keys per query tile, a key tail in the last; the counters reset by the call
    _v2_row(f"v2-fused-fresh-{IDS[_dt]}", ["fa_fwd_kernel" + FUSED], (2, 2, 500, 64), _dt,
            dict(kv_tiles_per_block=2, blocks_per_workgroup=1), fresh_ws=True, plan=(4, 1, 4))
    # ... a zeroed workspace and the caller's word for it: no reset, the counters left at zero
    _v2_row(f"v2-fused-zeroed-{IDS[_dt]}", ["fa_fwd16_kernel" + FUSED], (1, 3, 512, 128), _dt,
            dict(kv_tiles_per_block=2, blocks_per_workgroup=1), zeroed=True, plan=(4, 1, 4))
# key blocks of 4096 keys: the launcher hands the partials over arrival-first (fa_capi.cpp:
# kv_per_split >= 4096), the workgroup that arrives first polls the tile's counter
_v2_row("v2-arrive-first", ["fa_fwd16_kernel" + FUSED], (1, 1, 8192, 128), BF,
        dict(kv_tiles_per_block=64, blocks_per_workgroup=1), fresh_ws=True, plan=(2, 1, 2))
_v2_row("v2-fused-walk", ["fa_fwd16_chain_kernel<fused walk>"],
        lambda: (1, chain_cases(_cus())["walk"][0], chain_cases(_cus())["walk"][2], 128), BF,
        dict(kv_tiles_per_block=4, blocks_per_workgroup=1), fresh_ws=True, plan=(2, 1, 2))
_v2_row("v2-fp64", ["fa_fwd64_kernel<partial>", "fa_combine64_kernel"], (1, 2, 100, 64), torch.float64,
        dict(kv_tiles_per_block=2), fresh_ws=True)


def _partial_data(seed):
    x = _qkv("partial-combine", seed, 2, 2, 2, 192, 64, BF)
    # two key shards of 96 keys, each contiguous: [W, B, H, 96, d]
    return {"q": x["q"], "k": torch.stack([x["k"][:, :, :96], x["k"][:, :, 96:]]).contiguous(),
            "v": torch.stack([x["v"][:, :, :96], x["v"][:, :, 96:]]).contiguous(), "_k": x["k"], "_v": x["v"]}


def _partial_call(b, x):
    ops = _ops()
    for j in range(2):
        ops.attention_partial(b["q"], b["k"][j], b["v"][j], partial_dtype=ops.PARTIAL_FP16_SCALED,
                              o_part=x["o_part"][j:j + 1], lse=x["lse"][j:j + 1])
    return ops.combine(x["o_part"], x["lse"], 2, 2, BF, out=x["out"])


_row("partial-combine", [["fa_fwd_kernel<partial>"], ["fa_fwd_kernel<partial>"], ["fa_combine_kernel"]], _partial_data,
     _partial_call, lambda out, x: gate_mha(out, ref_mha(x["q"], x["_k"], x["_v"]), BF),
     lambda dev: {"o_part": torch.empty(2, 4, 192, 64, dtype=HF, device=dev),
                  "lse": torch.empty(2, 4, 192, 2, dtype=torch.float32, device=dev),
                  "out": torch.empty(2, 2, 192, 64, dtype=BF, device=dev)})

# decode: B = 3, H / H_kv = 4 / 2, 200 keys in four splits of one 64-key tile (the last holds 8)
DEC = dict(B=3, H=4, Hkv=2, Lk=200, ns=4)
# per seed: a 0, the full length and one in between, in another order
DEC_LENS = ((200, 0, 37), (0, 77, 200), (129, 200, 0), (200, 1, 0))


def _decode_row(d, Lq, dtype):
    name = f"decode-d{d}-Lq{Lq}-{IDS[dtype]}"
    B, H, Hkv, Lk, ns = (DEC[n] for n in ("B", "H", "Hkv", "Lk", "ns"))

    def data(seed):
        g = _gen(name, seed)
        q = torch.randn(B, H, Lq, d, generator=g).to(dtype)
        k, v = (torch.randn(B, Hkv, Lk, d, generator=g).to(dtype) for _ in range(2))
        return {"q": q, "k": k, "v": v, "seqlens": torch.tensor(DEC_LENS[seed % len(DEC_LENS)], dtype=torch.int32)}

    def call(b, x):
        return _ops().attention_decode(b["q"], b["k"], b["v"], seqlens_k=b["seqlens"], causal=True, num_splits=ns,
                                       out=x.get("out"), workspace=x.get("workspace"))

    def check(out, x):
        ref = decode_ref(*(x[n].double().numpy() for n in "qkv"), x["seqlens"].tolist(), True)
        test_decode._gate(out, ref, dtype, name, quiet=True)

    def scratch(dev):
        nbytes = _ops().decode_plan(B, H, Hkv, Lq, Lk, d, ns, dtype, cus=_cus())[2]
        return {"out": torch.empty(B, H, Lq, d, dtype=dtype, device=dev),
                "workspace": torch.empty(nbytes, dtype=torch.uint8, device=dev)}

    _row(name, [["fa_decode_kernel<16 rows>", "fa_decode_combine_kernel"]], data, call, check, scratch, fresh_ws=True)
    return name


DECODE_ROWS = [_decode_row(d, Lq, BF) for d in (64, 128) for Lq in (1, 4)] + [_decode_row(64, 1, HF), _decode_row(128, 4, HF)]

# paged decode: pages of 64 keys, four pages per sequence out of a pool of 15, 200 keys at most
PAGED = dict(B=3, H=4, Hkv=2, Lq=4, d=128, ps=64, P=4, nblk=15, Lk=200, ns=4)


def _paged_data(seed):
    c = PAGED
    g = _gen("paged", seed)
    q = torch.randn(c["B"], c["H"], c["Lq"], c["d"], generator=g).to(BF)
    kc, vc = (torch.randn(c["B"], c["Hkv"], c["P"] * c["ps"], c["d"], generator=g).to(BF) for _ in range(2))
    table = torch.randperm(c["nblk"], generator=g)[:c["B"] * c["P"]].reshape(c["B"], c["P"]).to(torch.int32)
    pools = []
    for cache in (kc, vc):  # the pages moved to where this seed's table says; the unused blocks hold noise
        pool = torch.randn(c["nblk"], c["ps"], c["Hkv"], c["d"], generator=g).to(BF)
        pages = cache.reshape(c["B"], c["Hkv"], c["P"], c["ps"], c["d"]).permute(0, 2, 3, 1, 4)  # [B, P, ps, Hkv, d]
        pool[table.reshape(-1).long()] = pages.reshape(-1, c["ps"], c["Hkv"], c["d"])
        pools.append(pool)
    return {"q": q, "k_cache": pools[0], "v_cache": pools[1], "table": table,
            "seqlens": torch.tensor(DEC_LENS[seed % len(DEC_LENS)], dtype=torch.int32), "_k": kc, "_v": vc}


def _paged_check(out, x):
    ref = decode_ref(x["q"].double().numpy(), x["_k"][:, :, :PAGED["Lk"]].double().numpy(),
                     x["_v"][:, :, :PAGED["Lk"]].double().numpy(), x["seqlens"].tolist(), True)
    test_decode._gate(out, ref, BF, "paged", quiet=True)


def _paged_scratch(dev):
    c = PAGED
    nbytes = _ops().decode_plan(c["B"], c["H"], c["Hkv"], c["Lq"], c["Lk"], c["d"], c["ns"], BF, cus=_cus())[2]
    return {"out": torch.empty(c["B"], c["H"], c["Lq"], c["d"], dtype=BF, device=dev),
            "workspace": torch.empty(nbytes, dtype=torch.uint8, device=dev)}


_row("paged", [["fa_decode_kernel<16 rows, paged>", "fa_decode_combine_kernel"]], _paged_data,
     lambda b, x: _ops().attention_decode_paged(b["q"], b["k_cache"], b["v_cache"], b["table"], seqlens_k=b["seqlens"],
                                                max_seqlen_k=PAGED["Lk"], causal=True, num_splits=PAGED["ns"],
                                                out=x.get("out"), workspace=x.get("workspace")),
     _paged_check, _paged_scratch, fresh_ws=True)

# varlen: one fused QKV projection [T, (H + 2 H_kv) d] read in place; an empty sequence, a single
# row, one past half a tile, one past a whole 128-row query tile; every seed the same total
VAR = dict(H=4, Hkv=2, d=64, msl=200)
VAR_LENS = ((0, 200, 65, 1, 130), (130, 1, 200, 0, 65), (65, 0, 1, 130, 200), (200, 130, 0, 65, 1))
VAR_T = sum(VAR_LENS[0])


def _varlen_data(seed):
    lens = VAR_LENS[seed % len(VAR_LENS)]
    assert sum(lens) == VAR_T and max(lens) <= VAR["msl"]
    qkv = torch.randn(VAR_T, (VAR["H"] + 2 * VAR["Hkv"]) * VAR["d"], generator=_gen("varlen", seed)).to(BF)
    return {"qkv": qkv, "cu": torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)}


def _varlen_views(qkv):
    heads = qkv.view(VAR_T, VAR["H"] + 2 * VAR["Hkv"], VAR["d"])
    return heads[:, :VAR["H"]], heads[:, VAR["H"]:VAR["H"] + VAR["Hkv"]], heads[:, VAR["H"] + VAR["Hkv"]:]


def _varlen_call(b, x):
    q, k, v = _varlen_views(b["qkv"])
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    return _ops().attention_varlen(q, k, v, b["cu"], VAR["msl"], causal=True, out=x["out"])


def _varlen_check(out, x):
    q, k, v = (t.double().numpy() for t in _varlen_views(x["qkv"]))
    ref, owned = varlen_ref(q, k, v, x["cu"].tolist(), VAR["msl"], True)
    assert owned.all()  # every row belongs to a sequence: the whole output is compared
    test_varlen._gate(out, ref, BF, "varlen")


_row("varlen", [["fa_fwd_kernel<final, varlen, causal, gqa>"]], _varlen_data, _varlen_call, _varlen_check,
     lambda dev: {"out": torch.empty(VAR_T, VAR["H"], VAR["d"], dtype=BF, device=dev)})

ALL = sorted(ROWS)
CONTROL = ("v1-tail-d64", "v2-fused-fresh-bf16", "decode-d128-Lq4-bf16", "paged", "varlen")
NO_ALLOC = DECODE_ROWS + ["paged"] + [n for n in ALL if n.startswith("v2-fused-") or n == "v2-arrive-first"]
CAPTURED = DECODE_ROWS + ["paged", "varlen", "v1-causal-gqa", "v1-chain", "v1-chain-gqa"] + [
    n for n in ALL if n.startswith(("v2-fused-fresh", "v2-fused-zeroed"))]
OTHER_DEVICE = ("decode-d128-Lq4-bf16", "paged", "varlen", "v2-fused-fresh-bf16", "v1-chain")
PAIRS = (("v2-fused-fresh-bf16", "v2-fused-zeroed-bf16"), ("decode-d128-Lq4-bf16", "paged"),
         ("v1-chain", "v2-arrive-first"), ("v1-chain", "v1-chain"), ("varlen", "decode-d64-Lq1-bf16"))


# ----------------------------------------------------------------------------------------
# the harness
# ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=8)
def _data(name, seed):
    """The row's host data of one seed; shared, nobody writes to it."""
    return ROWS[name].data(seed)


class Live:
    """A row's static device tensors: bufs (the inputs the call reads) and x (out, workspace)."""

    def __init__(self, name, dev, seed=0, scratch=True):
        self.row, self.dev = ROWS[name], dev
        self.bufs = {n: torch.empty_like(t, device=dev) for n, t in _data(name, seed).items() if not n.startswith("_")}
        self.x = self.row.scratch(dev) if scratch else {}
        self.poison()

    def stage(self, seed):
        """Device copies of one seed's inputs: the sources of put()."""
        return {n: _data(self.row.name, seed)[n].to(self.dev) for n in self.bufs}

    def put(self, staged):
        for n, t in self.bufs.items():
            t.copy_(staged[n])

    def poison(self):
        """NaN in every floating-point input and result buffer, zero in the lengths, tables and
        offsets (all valid), 0xff in a workspace the library resets itself."""
        for n, t in list(self.bufs.items()) + list(self.x.items()):
            if t.is_floating_point():
                t.fill_(float("nan"))
            elif t.dtype == torch.int32:
                t.zero_()
        if self.row.fresh_ws and "workspace" in self.x:
            self.x["workspace"].fill_(0xff)

    def run(self):
        return self.row.call(self.bufs, self.x)


def _names(kl):
    return [[part.split(" [grid")[0] for part in call.split(" + ")] for call in kl]


EAGER = {}


def eager(name, seed=0):
    """The row's result on cuda:0, default stream, synchronised before and after: the kernel
    names asserted, the result inside the fp64 gate.  Computed once per (row, seed), as bits on
    the host; read-only."""
    if (name, seed) not in EAGER:
        ops = _ops()
        dev = torch.device("cuda", 0)
        live = Live(name, dev, seed)
        live.put(live.stage(seed))
        torch.cuda.synchronize()
        with ops.launched_kernels() as kl:
            out = live.run()
        torch.cuda.synchronize()
        assert _names(kl) == ROWS[name].kernels, (name, kl)
        bits = out.clone().cpu()
        print(f"{name} seed {seed}: {' | '.join(kl)}")
        if seed == 0 or name not in HEAVY:
            ROWS[name].check(bits, _data(name, seed))
        EAGER[name, seed] = bits
    return EAGER[name, seed]


def _differ(got, want):
    got = got.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return got, got.view(INT[got.dtype]) != want.contiguous().view(INT[want.dtype])


def assert_bits(got, want, name, what):
    got, ne = _differ(got, want)
    if ne.any():
        at = tuple(ne.nonzero()[0].tolist())
        pytest.fail(f"{name} ({' + '.join(sum(ROWS[name].kernels, []))}) {what}: {int(ne.sum())} of {ne.numel()} elements "
                    f"differ from the eager result, first at {at}: got {got[at].item()!r}, want {want[at].item()!r}")


@functools.lru_cache(maxsize=None)
def _delay_fn():
    """A function that queues about DELAY_MS of work on the current stream."""
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return max(e0.elapsed_time(e1), 1e-3)

    if hasattr(torch.cuda, "_sleep"):
        cycles = int(DELAY_MS * 1_000_000 / timed(lambda: torch.cuda._sleep(1_000_000))) + 1
        return lambda: torch.cuda._sleep(cycles)
    a = torch.randn(2048, 2048, device="cuda")
    n = int(DELAY_MS / timed(lambda: a @ a)) + 1

    def chain():
        b = a
        for _ in range(n):
            b = a @ b
    return chain


def _wait(stream, what):
    """stream.synchronize() that reports a hang instead of sitting in it."""
    t0 = time.monotonic()
    while not stream.query():
        if time.monotonic() - t0 > WAIT_S:
            pytest.fail(f"{what}: the stream had not finished after {WAIT_S} s")
        time.sleep(0.0005)
    stream.synchronize()


def _runs_beside(a, b):
    """True when work queued on stream b does not wait for a delay queued on stream a."""
    delay = _delay_fn()
    x = torch.zeros(64, device=a.device)
    ev = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        delay()
    with torch.cuda.stream(b):
        x.add_(1)
        ev.record()
    t0 = time.monotonic()
    ev.synchronize()
    beside = time.monotonic() - t0 < DELAY_MS / 4 * 1e-3
    torch.cuda.synchronize()
    return beside


@functools.lru_cache(maxsize=None)
def _side_streams(gpu):
    """Two side streams that run beside the default stream and beside each other.  The runtime
    multiplexes its streams onto a few hardware queues (four by default), and two streams that
    share a queue run in submission order: a launch on the wrong stream would then still find
    its inputs ready and the test would prove nothing (measured: the control, below, matched for
    one row in four with a fresh stream per test).  So the streams are chosen once, with plain
    torch work, from at most twelve candidates; the library is not involved."""
    default, picked = torch.cuda.default_stream(gpu), []
    for _ in range(12):
        s = torch.cuda.Stream(gpu)
        if all(_runs_beside(s, o) and _runs_beside(o, s) for o in [default] + picked):
            picked.append(s)
            if len(picked) == 2:
                return tuple(picked)
    pytest.fail("no two side streams that run beside the default stream and each other")


def _behind_a_delay(name, gpu, call_on_side_stream):
    """Part 1's harness.  The default stream idle, the inputs stale; on a side stream a delay and
    the copies that bring the real inputs; then the call -- on the side stream too, or (the
    control) on the default stream -- and a clone on the call's stream.  No device synchronise
    until everything is queued."""
    delay = _delay_fn()
    live = Live(name, gpu)
    staged = live.stage(0)
    s = _side_streams(gpu)[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay()
        live.put(staged)
        if call_on_side_stream:
            got = live.run().clone()
    if call_on_side_stream:
        _wait(s, name)  # that stream only
    else:
        got = live.run().clone()
        torch.cuda.synchronize()
    return got


# ----------------------------------------------------------------------------------------
# part 1: the caller's stream is the stream
# ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ALL)
def test_eager_baseline_is_inside_the_fp64_gate(gpu, name):
    """The table itself: every row launches the kernels it names and its eager result passes
    the fp64 gate of the file that owns its reference."""
    eager(name)


@pytest.mark.parametrize("name", ALL)
def test_call_runs_on_the_callers_stream(gpu, name):
    want = eager(name)
    assert_bits(_behind_a_delay(name, gpu, True), want, name, "on a side stream behind a delay")


@pytest.mark.parametrize("name", CONTROL)
def test_control_call_on_another_stream_reads_stale_inputs(gpu, name):
    """Planted defect: the call on the default stream while its inputs sit behind the delay on
    the side stream.  It reads the stale (valid) inputs, so the comparison must reject it; if it
    does not, the delay is too short."""
    want = eager(name)
    got, ne = _differ(_behind_a_delay(name, gpu, False), want)
    print(f"control {name}: {int(ne.sum())} of {ne.numel()} elements differ")
    assert ne.any(), f"{name}: the control matched -- {DELAY_MS} ms of delay did not hold the inputs back"


@pytest.mark.parametrize("name", NO_ALLOC)
def test_call_with_out_and_workspace_allocates_nothing(gpu, name):
    want = eager(name)
    live = Live(name, gpu)
    live.put(live.stage(0))
    live.run()  # warm-up: the one-time attribute and device queries
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(gpu)["allocation.all.allocated"]
    out = live.run()
    after = torch.cuda.memory_stats(gpu)["allocation.all.allocated"]
    torch.cuda.synchronize()
    assert after == before, f"{name}: {after - before} allocations during the call"
    assert out is live.x["out"]
    assert_bits(out, want, name, "with out and workspace given")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _capi_decode(live, stream):
    b, x = live.bufs, live.x
    B, H, Lq, d = b["q"].shape
    return L.lib().fa_fwd_decode(_ptr(b["q"]), _ptr(b["k"]), _ptr(b["v"]), _ptr(x["out"]), _ptr(b["seqlens"]), B, H,
                                 DEC["Hkv"], Lq, DEC["Lk"], d, None, 1.0 / d ** 0.5, L.FA_FWD_CAUSAL, DEC["ns"],
                                 _ptr(x["workspace"]), x["workspace"].numel(), L.FA_DTYPE_BF16, stream)


def _capi_v2(live, stream):
    b, x = live.bufs, live.x
    B, H, L_, d = b["q"].shape
    return L.lib().fa_fwd_v2_ex(_ptr(b["q"]), _ptr(b["k"]), _ptr(b["v"]), _ptr(x["out"]), B, H, L_, d, 32, 32, 2, 1,
                                _ptr(x["workspace"]), x["workspace"].numel(), None, None, None, 1.0 / d ** 0.5,
                                L.FA_DTYPE_BF16, L.FA_DTYPE_FP16_SCALED, stream)


@pytest.mark.parametrize("name,entry", (("decode-d128-Lq4-bf16", _capi_decode), ("v2-fused-fresh-bf16", _capi_v2)),
                         ids=("fa_fwd_decode", "fa_fwd_v2_ex"))
def test_c_abi_on_an_explicit_side_stream(gpu, name, entry):
    """The C entry points handed a side stream's handle while the default stream is torch's
    current one: the same bits after synchronising that stream alone."""
    want = eager(name)
    delay = _delay_fn()
    live = Live(name, gpu)
    staged = live.stage(0)
    s = _side_streams(gpu)[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay()
        live.put(staged)
    assert torch.cuda.current_stream(gpu) != s
    L.check(entry(live, ctypes.c_void_p(s.cuda_stream)))
    assert _names([L.last_kernels()]) == ROWS[name].kernels
    with torch.cuda.stream(s):
        got = live.x["out"].clone()
    _wait(s, name)
    assert_bits(got, want, name, "through the C ABI on a side stream")


# ----------------------------------------------------------------------------------------
# part 2: two streams at once
# ----------------------------------------------------------------------------------------


def _two_streams(gpu, names, scratch=True):
    wants = [eager(n, seed) for seed, n in enumerate(names)]  # the second problem with other data
    lives = [Live(n, gpu, seed, scratch) for seed, n in enumerate(names)]
    for seed, live in enumerate(lives):
        live.put(live.stage(seed))
    streams = _side_streams(gpu)
    torch.cuda.synchronize()
    got = [[], []]
    for _ in range(ROUNDS):
        for i, (live, s) in enumerate(zip(lives, streams)):
            with torch.cuda.stream(s):
                out = live.run()
                got[i].append(out.clone())
                out.fill_(float("nan"))  # a round that did not run leaves no earlier round's result behind
    for s, n in zip(streams, names):
        _wait(s, n)
    for i, n in enumerate(names):
        for r, o in enumerate(got[i]):
            assert_bits(o, wants[i], n, f"round {r} on stream {i}, beside {names[1 - i]}")


@pytest.mark.timeout(180, method="thread")
@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}+{b}" for a, b in PAIRS])
def test_two_streams_do_not_disturb_each_other(gpu, a, b):
    _two_streams(gpu, (a, b))


@pytest.mark.timeout(180, method="thread")
def test_two_streams_with_allocator_temporaries(gpu):
    """out and workspace left to the call: each stream's temporaries come from torch's allocator."""
    _two_streams(gpu, ("decode-d128-Lq4-bf16", "paged"), scratch=False)


# ----------------------------------------------------------------------------------------
# part 3: capture and replay
# ----------------------------------------------------------------------------------------


def _capture(gpu, live, call):
    """A warm-up call on a side stream, then ONE call captured on that stream alone."""
    s = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()
    torch.cuda.synchronize()
    live.poison()
    live.put(live.stage(0))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = call()
    return graph, out


@pytest.mark.parametrize("name", CAPTURED)
def test_graph_replay_follows_the_static_tensors(gpu, name):
    wants = [eager(name, seed) for seed in (1, 2, 3)]
    assert _differ(wants[0], wants[1])[1].any(), "rounds 1 and 2 ask for the same result"
    live = Live(name, gpu)
    live.put(live.stage(0))
    graph, out = _capture(gpu, live, live.run)
    for seed, want in zip((1, 2, 3), wants):
        live.put(live.stage(seed))  # new contents, the same tensors
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(out, want, name, f"replay {seed} after the static tensors were rewritten")


@pytest.mark.parametrize("name", [n for n in CAPTURED if n.startswith("v2-fused-zeroed")])
def test_graph_replays_leave_the_counters_at_zero(gpu, name):
    """workspace_zeroed=True: five replays on the same workspace, nothing touching it in between."""
    want = eager(name)
    live = Live(name, gpu)
    live.put(live.stage(0))
    graph, out = _capture(gpu, live, live.run)
    for r in range(5):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(out, want, name, f"replay {r} on the untouched workspace")


def test_graph_replay_rejects_lengths_copied_at_capture(gpu):
    """Planted defect: the captured call reads a clone of seqlens_k made at capture time, as a
    library that copied the lengths would.  Every replay after new lengths must be rejected."""
    name = "decode-d128-Lq4-bf16"
    wants = [eager(name, seed) for seed in (1, 2, 3)]
    live = Live(name, gpu)
    live.put(live.stage(0))
    torch.cuda.synchronize()
    frozen = dict(live.bufs, seqlens=live.bufs["seqlens"].clone())
    graph, out = _capture(gpu, live, lambda: ROWS[name].call(frozen, live.x))
    for seed, want in zip((1, 2, 3), wants):
        live.put(live.stage(seed))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        ne = _differ(out, want)[1]
        print(f"lengths frozen at capture, replay {seed}: {int(ne.sum())} of {ne.numel()} elements differ")
        assert ne.any(), f"replay {seed} with stale lengths passed the bitwise comparison"


# ----------------------------------------------------------------------------------------
# part 4: the tensor's device, not the current one
# ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", OTHER_DEVICE)
def test_tensors_on_another_device_than_the_current_one(gpu, name):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: tensors on cuda:1 while cuda:0 is the current device")
    want = eager(name)
    other = torch.device("cuda", 1)
    torch.cuda.set_device(0)
    live = Live(name, other)
    live.put(live.stage(0))
    torch.cuda.synchronize(other)
    with _ops().launched_kernels() as kl:
        out = live.run()
    assert torch.cuda.current_device() == 0
    torch.cuda.synchronize(other)
    assert out.device == other and _names(kl) == ROWS[name].kernels, (out.device, kl)
    assert_bits(out, want, name, "on cuda:1 with cuda:0 current")
    assert torch.cuda.current_device() == 0
