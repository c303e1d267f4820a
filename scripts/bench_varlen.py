#!/usr/bin/env python3
"""attention_varlen on ragged prefill batches against what the library offered before it, at
d = 128 bf16, H32 H_kv8, causal, timed with bench.py's own method (its time_step / clock_settle /
launched helpers), all forms in ONE process on one device, alternating windows, median of the
rounds.

    python scripts/bench_varlen.py [--steps 30 --warmup 10 --rounds 3 --out profiles/varlen_bench.json]

Per batch:
  (a)  attention_varlen(q, k, v, cu_seqlens, max_seqlen, causal=True)    token-packed [T, H, d]
  (b)  attention_v1(causal=True) on the batch padded to max_seqlen, [B, H, Lmax, d] made beforehand
  (b+) (b) with the pack-to-padded copy of q, k, v and the unpack of o timed as well
  (c)  attention_v1(causal=True) once per sequence, on contiguous per-sequence tensors made
       beforehand (the copy out of the packed layout is NOT timed: the form's best case)
  (d)  torch scaled_dot_product_attention(is_causal=True) on the padded batch, K / V expanded to H
       heads beforehand (flash / memory-efficient backends; an error is recorded, not hidden)
Batches: (i) 16 x 4096 equal lengths; (ii) 16 sequences from 256 to 8192, a fixed seeded list;
(iii) 256 sequences of 128..512.  Also recorded: the 128-row x 64-key tiles walked by (a) and by
(b), and the largest |(a) - (b)| over the rows that exist.  No ratio is fixed in advance: the
numbers are written down whatever they are.  Needs a ROCm GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HKV, D = 32, 8, 128
BQ, BK = 128, 64


def batches():
    import numpy as np
    r2 = np.random.RandomState(2).randint(256, 8193, size=16)
    r2[0], r2[-1] = 256, 8192
    r3 = np.random.RandomState(3).randint(128, 513, size=256)
    return (("i", "16 x 4096", [4096] * 16), ("ii", "16 sequences 256..8192", [int(x) for x in r2]),
            ("iii", "256 sequences 128..512", [int(x) for x in r3]))


def causal_tiles(n):
    """KV tiles one head of a causal sequence of n rows walks: per query tile, the keys up to it."""
    return sum((min((qt + 1) * BQ, n) + BK - 1) // BK for qt in range((n + BQ - 1) // BQ))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="alternating windows of every form; the median is reported")
    ap.add_argument("--only", default="", help="comma-separated batch names (i, ii, iii); default all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_bench.json"))
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    import bench
    from exploring_flash_attention_amd import ops

    assert torch.cuda.is_available(), "bench_varlen.py needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    result = {"method": "bench.py time_step (device events around --steps back-to-back calls after --warmup "
                        "untimed ones and a 0.25 s clock settle), the forms alternating in one process, "
                        "median of --rounds windows; window_spread_ms = the largest max - min over a form's windows",
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "dtype": "bf16",
              "H": H, "H_kv": HKV, "d": D, "causal": True,
              "box": {"device": props.name, "compute_units": props.multi_processor_count,
                      "torch": torch.__version__, "hip": torch.version.hip},
              "cases": []}
    if os.path.exists(args.out) and args.only:  # a run split over several calls keeps what it has
        with open(args.out) as f:
            old = json.load(f)
        result["cases"] = [c for c in old.get("cases", []) if c["batch"] not in args.only.split(",")]

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    def ms(step):
        _, ev = bench.time_step(torch, step, args.steps, args.warmup, lambda: None)
        return ev / args.steps

    for name, desc, lens in batches():
        if args.only and name not in args.only.split(","):
            continue
        B, Lmax, T = len(lens), max(lens), sum(lens)
        cu_host = np.concatenate([[0], np.cumsum(lens)])
        g = torch.Generator(device=dev).manual_seed(1234)
        q = torch.randn(T, H, D, device=dev, dtype=torch.bfloat16, generator=g)
        k = torch.randn(T, HKV, D, device=dev, dtype=torch.bfloat16, generator=g)
        v = torch.randn(T, HKV, D, device=dev, dtype=torch.bfloat16, generator=g)
        cu = torch.tensor(cu_host.tolist(), dtype=torch.int32, device=dev)
        out = torch.empty_like(q)
        # the padded batch and the token -> (sequence, position) map of the pack / unpack copies
        bidx = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(lens, device=dev))
        pos = torch.arange(T, device=dev) - cu[:-1].long()[bidx]
        qp = torch.zeros(B, H, Lmax, D, device=dev, dtype=torch.bfloat16)
        kp, vp = (torch.zeros(B, HKV, Lmax, D, device=dev, dtype=torch.bfloat16) for _ in range(2))
        op = torch.empty_like(qp)
        ounp = torch.empty_like(q)

        def pack():
            qp[bidx, :, pos] = q
            kp[bidx, :, pos] = k
            vp[bidx, :, pos] = v

        pack()
        seqs = [tuple(t[int(cu_host[b]):int(cu_host[b + 1])].transpose(0, 1)[None].contiguous() for t in (q, k, v))
                for b in range(B)]
        seq_out = [torch.empty_like(s[0]) for s in seqs]
        ke, ve = kp.repeat_interleave(H // HKV, 1), vp.repeat_interleave(H // HKV, 1)

        def step_a():
            ops.attention_varlen(q, k, v, cu, Lmax, causal=True, out=out)

        def step_b():
            ops.attention_v1(qp, kp, vp, out=op, causal=True)

        def step_bcopy():
            pack()
            ops.attention_v1(qp, kp, vp, out=op, causal=True)
            ounp.copy_(op[bidx, :, pos])

        def step_c():
            for (qs, ks, vs), os_ in zip(seqs, seq_out):
                ops.attention_v1(qs, ks, vs, out=os_, causal=True)

        def step_d():
            with torch.nn.attention.sdpa_kernel([torch.nn.attention.SDPBackend.FLASH_ATTENTION,
                                                 torch.nn.attention.SDPBackend.EFFICIENT_ATTENTION]):
                torch.nn.functional.scaled_dot_product_attention(qp, ke, ve, is_causal=True)

        steps = {"a": step_a, "b": step_b, "b_with_copy": step_bcopy, "c": step_c, "d": step_d}
        sdpa_error = None
        try:
            step_d()
            torch.cuda.synchronize()
        except Exception as e:  # recorded below
            sdpa_error = f"{type(e).__name__}: {str(e)[:200]}"
            del steps["d"]
        labels = {"a": bench.launched(ops, step_a), "b": bench.launched(ops, step_b)}
        step_a()
        step_b()
        diff = float((out.float() - op[bidx, :, pos].float()).abs().max())
        bench.clock_settle(torch, step_b, 0.25)
        times = {n: [] for n in steps}
        for _ in range(args.rounds):
            for n in steps:
                times[n].append(ms(steps[n]))
        med = {n: statistics.median(t) for n, t in times.items()}
        spread = max(max(t) - min(t) for t in times.values())
        tiles_a = H * sum(causal_tiles(n) for n in lens)
        tiles_b = H * B * causal_tiles(Lmax)
        rec = {"batch": name, "what": desc, "B": B, "total_tokens": T, "max_seqlen": Lmax,
               "lens_min_median_max": [min(lens), int(statistics.median(lens)), Lmax],
               "a_varlen_ms": round(med["a"], 5), "b_padded_ms": round(med["b"], 5),
               "b_padded_with_pack_copy_ms": round(med["b_with_copy"], 5), "c_per_sequence_ms": round(med["c"], 5),
               "d_torch_sdpa_padded_ms": round(med["d"], 5) if "d" in med else None, "d_error": sdpa_error,
               "windows_ms": {n: [round(x, 5) for x in t] for n, t in times.items()},
               "window_spread_ms": round(spread, 5),
               "spread_ms": {n: round(max(t) - min(t), 5) for n, t in times.items()},
               "a_over_b": round(med["a"] / med["b"], 4), "a_over_b_with_copy": round(med["a"] / med["b_with_copy"], 4),
               "a_over_c": round(med["a"] / med["c"], 4),
               "kv_tiles_a": tiles_a, "kv_tiles_b": tiles_b, "tiles_a_over_b": round(tiles_a / tiles_b, 4),
               "a_grid_items": B * H * ((Lmax + BQ - 1) // BQ),
               "a_items_that_run": H * sum((n + BQ - 1) // BQ for n in lens),
               "a_kernel": labels["a"], "b_kernel": labels["b"], "max_abs_a_minus_b": diff,
               "a_tflops": round(4.0 * tiles_a * BQ * BK * D / (med["a"] * 1e-3) / 1e12, 1),
               "b_tflops": round(4.0 * tiles_b * BQ * BK * D / (med["b"] * 1e-3) / 1e12, 1)}
        result["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        write()
        del q, k, v, out, qp, kp, vp, op, ounp, seqs, seq_out, ke, ve, steps
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
