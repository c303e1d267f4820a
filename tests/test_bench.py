"""bench.py's host-side logic on CPU: the C5 watchdog fails the run, the head sample, the
usable-core count, the heads --dump-outputs writes; on the GPU, what a plain run does."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_watchdog_exits_nonzero_and_prints_partial_line():
    code = (
        "import sys, time; sys.path.insert(0, %r); import bench\n"
        "bench.start_watchdog(0.3, 0, lambda: {'metric': 'm', 'extra': {'c5_splitkv_dist': {'error': 'hung'}}})\n"
        "time.sleep(30)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert '"error": "hung"' in r.stdout and "watchdog fired" in r.stderr


def test_watchdog_cancelled_is_silent():
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "d = bench.start_watchdog(0.5, 1, lambda: None); d.cancel(); time.sleep(1.0)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""


def test_sample_heads_and_host_cores():
    sys.path.insert(0, ROOT)
    import bench
    hs = bench.sample_heads(32, 8)
    assert len(hs) == 16 and hs[0] == (0, 0) and hs[-1] == (31, 7)
    usable, total = bench.host_cores()
    assert 1 <= usable <= total == os.cpu_count()
    assert bench.cpu_model()


def test_gpus_request_beyond_the_node_fails_loudly():
    """`bench.py --gpus 2` with no launcher on a node with fewer GPUs (this container has none)
    exits non-zero with a message -- never a one-GPU line labelled n_gpus 1."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == "" and "--gpus 2 requested" in r.stderr


def test_world_size_disagreeing_with_gpus_is_an_error():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2 and "disagree" in r.stderr and r.stdout.strip() == ""


def test_spawn_ranks_starts_n_ranks_and_propagates_failure(tmp_path):
    """The launcher bench.py uses for --gpus N: N processes with RANK / WORLD_SIZE set, and a
    failing rank makes the whole launch fail (non-zero status)."""
    sys.path.insert(0, ROOT)
    import bench
    script = tmp_path / "rank.py"
    script.write_text(
        "import os, sys\n"
        "r, w = os.environ['RANK'], os.environ['WORLD_SIZE']\n"
        "open(os.path.join(sys.argv[1], 'rank' + r), 'w').write(w)\n"
        "sys.exit(7 if sys.argv[2] == r else 0)\n")
    assert bench.spawn_ranks(3, str(script), [str(tmp_path), "-1"]) == 0
    assert sorted(p.name for p in tmp_path.glob("rank[0-9]")) == ["rank0", "rank1", "rank2"]
    assert all((tmp_path / f"rank{i}").read_text() == "3" for i in range(3))
    for p in tmp_path.glob("rank[0-9]"):
        p.unlink()
    assert bench.spawn_ranks(2, str(script), [str(tmp_path), "1"]) != 0


def test_extra_shapes_split_where_the_library_splits():
    """The split-KV bench extras: the two low-parallelism shapes are planned with more than one
    partial per query tile by the library (on the MI355X's 256 CUs), their `unsplit` twins
    with one."""
    sys.path.insert(0, ROOT)
    import bench
    from exploring_flash_attention_amd import ops
    shapes = {s[0]: s for s in bench.EXTRA_SHAPES}
    for base, ppt in (("b1h1_l16k", 4), ("b1h2_l4k", 4)):
        _, B, H, L, d, _, kvt, grp = shapes[base + "_splitkv"]
        assert grp is None and ops.v2_split_plan(B, H, L, d, kvt)[2] == ppt
        _, B, H, L, d, _, kvt, grp = shapes[base + "_unsplit"]
        blocks = ops.v2_split_plan(B, H, L, d, kvt)[0]
        assert grp == "all" and ops.v2_split_plan(B, H, L, d, kvt, blocks_per_workgroup=blocks)[2] == 1


def test_splitkv_scaling_field_at_mocked_two_ranks():
    """At N > 1 the C5 split-KV measurement (north_star's multi-GPU row) is a top-level field of
    the bench line, carrying ms, whole-job rate, frac and the exchange's own ms / GB/s."""
    sys.path.insert(0, ROOT)
    import bench
    c5 = {"ms": 15.0, "tflops": 2345.6, "frac": 0.469, "ranks": 2, "exchange": "pairwise send/recv",
          "breakdown_max_over_ranks": {"partial_ms": 14.1, "combine_ms": 0.4, "exchange_ms": 3.2,
                                       "exchange_gbps": 167.8, "exchange_bytes_per_rank": 537_000_000}}
    rec = bench.splitkv_scaling_field(c5, 2)
    assert rec["ranks"] == 2 and rec["ms"] == 15.0 and rec["frac"] == 0.469
    assert rec["value"] == 2345600.0 and rec["exchange_ms"] == 3.2 and rec["exchange_gbps"] == 167.8
    err = bench.splitkv_scaling_field({"error": "no result within 240 s", "ranks": 2}, 2)
    assert err["error"].startswith("no result") and "ms" not in err


def test_kernel_labels_come_from_the_library():
    """bench.py names the kernels the library reports having launched (fa_last_kernels through
    ops.launched_kernels), in call order without repeats -- no restated launch rule to drift
    from fa_fwd.hip."""
    import contextlib
    sys.path.insert(0, ROOT)
    import bench

    class FakeOps:
        @contextlib.contextmanager
        def launched_kernels(self):
            log = []
            self.log = log
            yield log

    ops = FakeOps()

    def step():  # a C5-like step: three partial chunks and a combine
        ops.log.extend(["fa_fwd16_kernel<partial, strided> [grid 256]"] * 3 + ["fa_combine_kernel [grid 64]"])
    assert bench.launched(ops, step) == "fa_fwd16_kernel<partial, strided> [grid 256] + fa_combine_kernel [grid 64]"
    assert bench.launched(ops, lambda: None) is None


def test_extra_traffic_records_are_labelled():
    """Every bench extra with a traffic entry reports measured bytes, the algorithmic bytes and
    the kernel the PMC pass measured."""
    import bench
    for name, B, H, L, d, *_ in bench.EXTRA_SHAPES:
        tr = bench.extra_traffic(name, B, H, L, d)
        if tr is None:
            continue
        assert tr["algorithmic_bytes"] == 8 * B * H * L * d
        assert tr["bytes_per_launch"] > 0 and tr["ratio"] > 0
        assert tr["kernel"] and tr["kernel"] != "(unlabelled)", name


def test_dump_heads_are_fixed_and_fit_the_budget():
    """--dump-outputs: the whole output where it fits 32 MiB of float32, else whole heads drawn
    by a fixed seed -- the same ones on every call, distinct, in batch order, within the budget."""
    import bench
    assert bench.DUMP_BYTES <= 64_000_000
    assert bench.dump_heads(2, 3, 200, 64) == [(b, h) for b in range(2) for h in range(3)]
    for cfg in ("c2", "c3", "c4", "c5"):
        c = bench.CONFIGS[cfg]
        B, H, L, d = c["B"], c["H"], c["L"], c["d"]
        hs = bench.dump_heads(B, H, L, d)
        assert hs == bench.dump_heads(B, H, L, d) and hs == sorted(set(hs))
        assert all(0 <= b < B and 0 <= h < H for b, h in hs)
        assert len(hs) == min(B * H, bench.DUMP_BYTES // (L * d * 4)) >= 1
    # N ranks share the budget
    assert len(bench.dump_heads(32, 8, 1024, 128, bench.DUMP_BYTES // 8)) == 8


def test_plain_and_full_arguments():
    """--full and --dump-outputs exist, both off by default; --steps 0 is refused before any work."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == ""


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_its_output(gpu, tmp_path, capsys, monkeypatch):
    """A plain `bench.py --gpus 1 --steps N --warmup W`: exactly W + N forwards after the one
    that names the kernel, none of the --full legs, one JSON line whose value follows from
    ms_per_step; --dump-outputs writes the last step's output -- float32, under 64 MB, the same
    bits on a second run, and the attention of the seeded inputs (bf16 build gate, test_gpu.GATE)."""
    import torch

    import bench
    from exploring_flash_attention_amd import ops

    def full_only(*a, **k):
        raise AssertionError("a --full leg ran in a plain benchmark run")
    for name in ("cpu_baseline", "cpu_baseline_openmp", "single_gpu_extras", "measured_ceiling", "output_check",
                 "c5_step", "c5_breakdown"):
        monkeypatch.setattr(bench, name, full_only)
    calls = []
    v1 = ops.attention_v1

    def counted_v1(*a, **k):
        calls.append(1)
        return v1(*a, **k)
    monkeypatch.setattr(ops, "attention_v1", counted_v1)
    N, W = 3, 2
    lines, outs = [], []
    for sub in ("a", "b"):
        del calls[:]
        bench.main(["--gpus", "1", "--steps", str(N), "--warmup", str(W), "--clock-warmup", "0",
                    "--dump-outputs", str(tmp_path / sub)])
        assert len(calls) == 1 + W + N
        printed = capsys.readouterr().out.strip().splitlines()
        assert len(printed) == 1
        lines.append(json.loads(printed[0]))
        assert [f.name for f in (tmp_path / sub).iterdir()] == ["out.npy"]
        outs.append(np.load(tmp_path / sub / "out.npy", allow_pickle=False))
    c = bench.CONFIGS["c3"]
    B, H, L, d = c["B"], c["H"], c["L"], c["d"]
    for line in lines:
        assert line["steps"] == N and line["warmup"] == W and line["n_gpus"] == 1
        assert line["unit"] == "GFLOP/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert line["metric"].startswith("flash-attn fwd GFLOP/s (B=32,H=8,L=1024,d=128")
        assert line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(bench.flops(B, H, L, d) / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
        assert line["cpu_baseline"] is None and "extra" not in line and "check" not in line
        assert "ceiling_measured" not in line["roofline"] and line["roofline"]["kernel"]
        assert line["outputs"]["file"] == "out.npy" and line["outputs"]["dtype"] == "float32"
    heads = bench.dump_heads(B, H, L, d)
    a, b = outs
    assert a.dtype == np.float32 and a.shape == (len(heads), L, d) and a.nbytes <= 64_000_000
    assert np.array_equal(a, b)
    q, k, v = bench._make_inputs(torch, gpu, B, H, L, d, seed=1234)
    for i in (0, len(heads) // 2, len(heads) - 1):
        bb, hh = heads[i]
        qq, kk, vv = (t[bb, hh].double() for t in (q, k, v))
        ref = (torch.softmax((qq @ kk.T) / d ** 0.5, dim=-1) @ vv).cpu().numpy()
        err = np.abs(a[i] - ref)
        big = np.abs(ref) > 1e-3
        assert err.max() <= 6e-3 and (err[big] / np.abs(ref[big])).mean() <= 1e-2, (bb, hh, err.max())
