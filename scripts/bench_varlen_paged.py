#!/usr/bin/env python3
"""attention_varlen_paged (chunked prefill against a block-table KV cache, read in place) and
kv_cache_append_paged against the forms the library had before them, at d = 128 bf16, H32 H_kv8,
causal, timed with bench.py's own method (time_step / clock_settle / launched), all forms in ONE
process on one device, alternating windows, median of the rounds.

    python scripts/bench_varlen_paged.py [--steps 20 --warmup 5 --rounds 3 --out profiles/varlen_paged_bench.json]

Per page size (64 / 128 / 256 keys, the pages shuffled over the pool), 16 sequences of 512 new tokens
each against 8192 keys (scripts/bench_varlen_kv.py's case a), and once a batch of mixed key lengths:
  paged          attention_varlen_paged(q, k_pool, v_pool, cu_q, 512, block_table, seqused_k, causal=True)
  contiguous     attention_varlen(cu_seqlens_k=, seqused_k=) on a padded [B, Lmax, H_kv, d] cache with
                 the SAME row stride (H_kv * d) -- paged / contiguous is the cost of paging alone
  gather         index_select of every sequence's pages into such a cache, then that call -- the only
                 form a caller with a paged cache had before
  append         kv_cache_append_paged of the 512 new tokens of every sequence
  append_paged   append, then the paged call (one prefill chunk of a serving engine)
Also recorded: whether the paged rows equal the contiguous call's bit for bit.  Acceptance is relative
to the existing paths: paged below gather at every page size; paged / contiguous with the windows'
spread beside it.  Needs a ROCm GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HKV, D = 32, 8, 128


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating windows of every form; the median is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_paged_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import bench
    from exploring_flash_attention_amd import ops

    assert torch.cuda.is_available(), "bench_varlen_paged.py needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    result = {"method": "bench.py time_step (device events around --steps back-to-back calls after --warmup "
                        "untimed ones and a 0.25 s clock settle), the forms alternating in one process, "
                        "median of --rounds windows; window_spread_ms = the largest max - min over the windows of "
                        "paged and contiguous",
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "dtype": "bf16",
              "H": H, "H_kv": HKV, "d": D, "causal": True,
              "box": {"device": props.name, "compute_units": props.multi_processor_count,
                      "torch": torch.__version__, "hip": torch.version.hip},
              "cases": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    def ms(step):
        _, ev = bench.time_step(torch, step, args.steps, args.warmup, lambda: None)
        return ev / args.steps

    def measure(steps, settle):
        bench.clock_settle(torch, settle, 0.25)
        times = {n: [] for n in steps}
        for _ in range(args.rounds):
            for n in steps:
                times[n].append(ms(steps[n]))
        return {n: statistics.median(t) for n, t in times.items()}, times

    def i32(x):
        return torch.tensor(x, dtype=torch.int32, device=dev)

    g = torch.Generator(device=dev).manual_seed(4321)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, dtype=torch.bfloat16, generator=g)

    B, L, C = 16, 8192, 512
    q = rnd(B * C, H, D)
    k_new, v_new = rnd(B * C, HKV, D), rnd(B * C, HKV, D)
    cache_k, cache_v = rnd(B, L, HKV, D), rnd(B, L, HKV, D)        # the padded cache: row stride H_kv * d
    cu_q = i32([b * C for b in range(B + 1)])
    cu_k = i32([b * L for b in range(B + 1)])
    out_p, out_c, out_g = (torch.empty_like(q) for _ in range(3))

    for what, lens_k in (("16 sequences, 512 new tokens each against 8192 keys", [L] * B),
                         ("mixed key lengths, 512 new tokens each",
                          [8192, 4096, 2048, 1024, 512, 6000, 3000, 777, 8192, 5000, 1536, 640, 7000, 2500, 1000, 8000])):
        su = i32(lens_k)
        for ps in ((64, 128, 256) if lens_k == [L] * B else (128,)):
            P = L // ps
            nb = B * P
            perm = torch.randperm(nb, device=dev, generator=g)
            table = perm.view(B, P).to(torch.int32).contiguous()
            pool_k, pool_v = torch.empty(nb, ps, HKV, D, device=dev, dtype=torch.bfloat16), None
            pool_v = torch.empty_like(pool_k)
            pool_k[perm] = cache_k.view(nb, ps, HKV, D)             # page p of sequence b -> block table[b, p]
            pool_v[perm] = cache_v.view(nb, ps, HKV, D)
            flat = table.flatten().long()

            def paged():
                ops.attention_varlen_paged(q, pool_k, pool_v, cu_q, C, table, su, causal=True, out=out_p)

            def contiguous(kc=cache_k, vc=cache_v, out=out_c):
                ops.attention_varlen(q, kc.view(B * L, HKV, D), vc.view(B * L, HKV, D), cu_q, C, causal=True, out=out,
                                     cu_seqlens_k=cu_k, max_seqlen_k=L, seqused_k=su)

            def gather():
                contiguous(pool_k.index_select(0, flat), pool_v.index_select(0, flat), out_g)

            def append():
                ops.kv_cache_append_paged(k_new, v_new, pool_k, pool_v, cu_q, C, table, su)

            def append_paged():
                append()
                paged()

            steps = {"paged": paged, "contiguous": contiguous, "gather": gather, "append": append,
                     "append_paged": append_paged}
            labels = {n: bench.launched(ops, f) for n, f in (("paged", paged), ("contiguous", contiguous),
                                                             ("append", append))}
            # (the append overwrote the last 512 keys of every sequence in the pool: put them back)
            pool_k[perm] = cache_k.view(nb, ps, HKV, D)
            pool_v[perm] = cache_v.view(nb, ps, HKV, D)
            paged(), contiguous(), gather()
            torch.cuda.synchronize()
            same = torch.equal(out_p, out_c) and torch.equal(out_p, out_g)
            med, times = measure(steps, contiguous)
            spread = max(max(times[n]) - min(times[n]) for n in ("paged", "contiguous"))
            rec = {"what": what, "B": B, "len_q": C, "len_k": lens_k if len(set(lens_k)) > 1 else lens_k[0],
                   "page_size": ps, "num_blocks": nb,
                   "paged_ms": round(med["paged"], 5), "contiguous_same_row_stride_ms": round(med["contiguous"], 5),
                   "gather_then_call_ms": round(med["gather"], 5), "append_ms": round(med["append"], 5),
                   "append_then_paged_ms": round(med["append_paged"], 5),
                   "windows_ms": {n: [round(x, 5) for x in t] for n, t in times.items()},
                   "window_spread_ms": round(spread, 5),
                   "paged_over_contiguous": round(med["paged"] / med["contiguous"], 4),
                   "spread_over_contiguous": round(spread / med["contiguous"], 4),
                   "gather_over_paged": round(med["gather"] / med["paged"], 3),
                   "paged_below_gather": bool(med["paged"] < med["gather"]),
                   "append_gbytes_per_s": round(4 * B * C * HKV * D * 2 / (med["append"] * 1e-3) / 1e9, 1),
                   "kernels": labels, "paged_equals_contiguous_and_gather_bitwise": bool(same)}
            result["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            write()
            del pool_k, pool_v
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
