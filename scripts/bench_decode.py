#!/usr/bin/env python3
"""KV-cache decode (ops.attention_decode) at d = 128 bf16 against what else serves the shape,
timed with bench.py's own method (its time_step / clock_settle / launched helpers), all forms in
ONE process on one device, alternating windows, the median of --rounds windows reported.

    python scripts/bench_decode.py [--steps 500 --warmup 300 --rounds 3 --out profiles/decode_bench.json]

Shapes: H32 H_kv8 Lk8192 with B in {1, 16, 64} at Lq = 1, and B16 at Lq = 4 causal.  Per shape:
  (a) attention_decode(q, k, v)                 k, v [B, H_kv, Lk, d], out and workspace given
  (b) attention_partial(q, k_exp, v_exp)        the one call that took Lq != Lk before decode: its
                                                single partial over the whole key range IS the
                                                answer; K / V expanded to H heads beforehand (not
                                                timed).  Lq = 1: the causal mask is moot.  Left
                                                out at Lq = 4 causal (it has no mask).
  (c) torch SDPA on the expanded K / V          (a bottom-right boolean mask at Lq = 4 causal)
  (d) a device-to-device copy of as many bytes as (a) must read (q, K and V once): the bandwidth
      ceiling of this process on this device, live
Acceptance: (a) beats (b) and (c) by more than the spread of the windows at every shape; (a)'s
bytes/s is recorded as a fraction of (d)'s.  Needs a ROCm GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (B, H, H_kv, Lq, Lk, d, causal)
SHAPES = ((1, 32, 8, 1, 8192, 128, False), (16, 32, 8, 1, 8192, 128, False), (64, 32, 8, 1, 8192, 128, False),
          (16, 32, 8, 4, 8192, 128, True))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3, help="alternating windows of every form; the median is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import bench
    from exploring_flash_attention_amd import ops

    assert torch.cuda.is_available(), "bench_decode.py needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    result = {"method": "bench.py time_step (device events around --steps back-to-back calls after --warmup "
                        "untimed ones and a 0.25 s clock settle), all forms alternating in one process",
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "dtype": "bf16",
              "box": {"device": props.name, "compute_units": props.multi_processor_count,
                      "torch": torch.__version__, "hip": torch.version.hip},
              "cases": []}

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    def ms(step):
        _, ev = bench.time_step(torch, step, args.steps, args.warmup, lambda: None)
        return ev / args.steps

    for B, H, Hkv, Lq, Lk, d, causal in SHAPES:
        G = H // Hkv
        q, _, _ = bench._make_inputs(torch, dev, B, H, Lq, d, seed=1234)
        _, k, v = bench._make_inputs(torch, dev, B, Hkv, 1, d, seed=4321, Lk=Lk)
        ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
        out = torch.empty_like(q)
        splits, kps, nbytes = ops.decode_plan(B, H, Hkv, Lq, Lk, d)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        read_bytes = (q.numel() + k.numel() + v.numel()) * 2
        src = torch.empty(read_bytes, dtype=torch.uint8, device=dev).random_(0, 255)
        dst = torch.empty_like(src)
        mask = None
        if causal:  # bottom-right aligned: row i sees keys j <= Lk - Lq + i
            j = torch.arange(Lk, device=dev)[None, :]
            mask = j <= (Lk - Lq + torch.arange(Lq, device=dev))[:, None]
        sdpa = torch.nn.functional.scaled_dot_product_attention
        steps = {"a": lambda: ops.attention_decode(q, k, v, causal=causal, out=out, workspace=ws),
                 "c": lambda: sdpa(q, ke, ve, attn_mask=mask),
                 "d": lambda: dst.copy_(src)}
        if not causal:
            o_part = torch.empty((1, B * H, Lq, d), dtype=torch.float32, device=dev)
            lse = torch.empty((1, B * H, Lq), dtype=torch.float32, device=dev)
            steps["b"] = lambda: ops.attention_partial(q, ke, ve, o_part=o_part, lse=lse)
        labels = {n: bench.launched(ops, steps[n]) for n in ("a", "b") if n in steps}
        # the forms agree (bf16 output of (a) against the fp32 partial of (b) and SDPA's output)
        oa = ops.attention_decode(q, k, v, causal=causal).float()
        err_c = float((oa - sdpa(q, ke, ve, attn_mask=mask).float()).abs().max())
        err_b = float((oa - steps["b"]()[0].view(B, H, Lq, d)).abs().max()) if "b" in steps else None
        del oa
        bench.clock_settle(torch, steps["a"], 0.25)
        order = [n for n in ("a", "b", "c", "d") if n in steps]
        times = {n: [] for n in order}
        for _ in range(args.rounds):
            for n in order:
                times[n].append(ms(steps[n]))
        med = {n: statistics.median(t) for n, t in times.items()}
        spread = max(max(t) - min(t) for n, t in times.items() if n != "d")
        a_gbs = read_bytes / (med["a"] * 1e-3) / 1e9
        d_gbs = read_bytes / (med["d"] * 1e-3) / 1e9
        rec = {"B": B, "H": H, "H_kv": Hkv, "Lq": Lq, "Lk": Lk, "d": d, "causal": causal,
               "splits": splits, "keys_per_split": kps, "workspace_bytes": nbytes,
               "a_decode_ms": round(med["a"], 5),
               "b_partial_expanded_ms": round(med["b"], 5) if "b" in med else None,
               "b_note": None if "b" in med else "left out: attention_partial has no causal mask",
               "c_sdpa_expanded_ms": round(med["c"], 5), "d_copy_ms": round(med["d"], 5),
               "windows_ms": {n: [round(x, 5) for x in t] for n, t in times.items()},
               "window_spread_ms": round(spread, 5),
               "a_beats_b": bool(med["b"] - med["a"] > spread) if "b" in med else None,
               "a_beats_c": bool(med["c"] - med["a"] > spread),
               "bytes_a_must_read": read_bytes, "a_read_GBps": round(a_gbs, 1), "d_copy_GBps": round(d_gbs, 1),
               "a_fraction_of_copy": round(a_gbs / d_gbs, 3),
               "a_kernel": labels["a"], "b_kernel": labels.get("b"),
               "max_abs_a_vs_b": err_b, "max_abs_a_vs_sdpa": err_c}
        result["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        write()
        del q, k, v, ke, ve, out, ws, src, dst, steps
        torch.cuda.empty_cache()

    bad = [r for r in result["cases"] if not (r["a_beats_c"] and r["a_beats_b"] is not False)]
    if bad:
        print("attention_decode does not beat (b) / (c) at", [(r["B"], r["Lq"], r["causal"]) for r in bad], file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
