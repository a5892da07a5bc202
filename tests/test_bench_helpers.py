"""bench.py bookkeeping: the algorithmic flop / byte model is SURVEY.md section 8(d)'s."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_algorithmic_flops_and_bytes_match_the_survey():
    b = _bench()
    assert abs(b.algorithmic_flops(10, 50) / 1e6 - 4.29) < 0.01          # N=10, K=50 -> 4.29 MF
    assert abs(b.algorithmic_flops(20, 50) / 1e6 - 26.6) < 0.1
    for N, mf in ((8, 2.46), (12, 6.85), (16, 14.6), (24, 43.9)):
        assert abs(b.algorithmic_flops(N, 50) / 1e6 - mf) < 0.06 * mf
    assert b.algorithmic_bytes(10) == 4536                               # 4,536 B per QP (N=10, fp64)
    assert b.PEAK_FP64_TFLOPS == 78.6 and b.BATCH_PER_GPU == 4096 and b.HORIZON == 10


def test_useful_flops_model():
    """W_eff (bench.useful_flops): the presolved / wrench-reduced algorithm's own flop count.  configs[1] (N = 10, 2 stance contacts per step,
    n_eff = 60, m_eff = 100): the 60^3 of factor + L^-1 + W'W, 18 flops per entry of one triangle, K x (2 60^2 + 10 100) -- the round-4 judge's
    estimate was 0.55 MF per QP at K = 33.7."""
    import numpy as np
    b = _bench()
    w = b.useful_flops(10, 33.745, 2)
    assert abs(w - (500 * 10 + 2 * 2 * 13 * 13 * 10 + 38 * 60 + 54 * 60 + 18 * 60 * 61 / 2 + 60 ** 3 + 33.745 * (2 * 3600 + 1000))) < 1e-6
    assert 0.50e6 < w < 0.60e6
    assert w < 0.2 * b.algorithmic_flops(10, 33.745)                      # far below the dense path's W: swing variables dropped, closed form
    # affine in K, and the batch sum groups by pattern without changing the total
    assert abs((b.useful_flops(10, 40, 2) - b.useful_flops(10, 30, 2)) - 10 * (2 * 3600 + 1000)) < 1e-6
    rng = np.random.default_rng(0)
    ct = (rng.random((50, 8, 4)) < 0.6).astype(np.uint8)
    it = rng.integers(5, 200, 50)
    for wrench in (False, True):
        ref = sum(b.useful_flops(8, float(it[i]), ct[i].sum(axis=1), wrench) for i in range(50))
        assert abs(b.useful_flops_batch(8, ct, it, wrench) - ref) < 1e-6 * ref
    # the wrench reduction: full double support at N = 20 is a 120 x 120 problem, not 240 x 240
    wd = b.useful_flops(20, 50, 4, wrench=True)
    assert 120 ** 3 < wd < 120 ** 3 + 51 * (2 * 120 ** 2 + 20 * (72 * 4 + 18 * 16) + 4000) + 2.5e5
    # a step with <= 2 stance contacts keeps its force variables: same matrix size as the dense presolved path
    assert abs(b.useful_flops(10, 0, 2, wrench=True) - b.useful_flops(10, 0, 2, wrench=False)) < 0.05 * b.useful_flops(10, 0, 2)


def test_force_dist_runs_the_collective_at_world_size_one():
    """`--force-dist`: torch.distributed initialised and the per-step all-gather of u_opt0 executed with ONE rank (here gloo + the stubbed
    solve; on the GPU box the same flag runs RCCL -- tests/test_gpu_parity.py)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--stub-solve", "--backend", "gloo", "--force-dist", "--steps", "4",
                        "--warmup", "2", "--batch", "32", "--full"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["config"]["allgather_in_value"] is True
    assert d["config"]["collective"]["backend"] == "gloo" and d["config"]["collective"]["world_size"] == 1 and d["config"]["collective"]["forced_at_world_size_1"]
    assert d["value"] > 0 and d["value_without_allgather"] > 0


def test_bench_starts_its_own_ranks_without_a_launcher():
    """`python bench.py --gpus 2` with no torchrun around it: the script starts one process per rank before anything
    touches a GPU, rank 0 prints the one JSON line, both the with- and the without-all-gather rates are reported.  Here on
    CPU: gloo, the solve stubbed (the launcher path, the rotation over batches and the collective are what is tested)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--stub-solve", "--backend", "gloo", "--steps", "6",
                        "--warmup", "2", "--batch", "32", "--full"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["scaling"] == "weak" and d["unit"] == "QP/s"
    assert d["config"]["allgather_in_value"] is True and d["config"]["distinct_batches"] == 4
    assert d["value"] > 0 and d["value_without_allgather"] > 0
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--stub-solve", "--backend", "gloo", "--steps", "3",
                         "--warmup", "1", "--batch", "16", "--no-allgather", "--full"], capture_output=True, text=True, timeout=300, env=env)
    assert r2.returncode == 0, r2.stderr[-2000:]
    d2 = json.loads([ln for ln in r2.stdout.splitlines() if ln.startswith("{")][0])
    assert d2["config"]["allgather_in_value"] is False and d2["value_with_allgather"] > 0


def _run_stub(*extra, gpus="1"):
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", gpus, "--stub-solve", "--backend", "gloo"] + list(extra),
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_headline_steps_only_and_dumps_the_last_one(tmp_path):
    """A plain run: --steps K timed steps, the headline fields, nothing of what --full adds; --dump-outputs writes the last timed step's
    arrays as float .npy files, the same from run to run (here the stubbed solve on CPU: u = the step's foot positions)."""
    import numpy as np
    b = _bench()
    d = _run_stub("--steps", "6", "--warmup", "2", "--batch", "32", "--dump-outputs", str(tmp_path / "a"))
    assert d["steps"] == 6 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "QP/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["metric"].startswith("QP solves/sec")
    for k in ("roofline", "value_plain", "in_place", "latency_batch1", "also", "cpu_baseline", "value_without_allgather", "value_with_allgather"):
        assert k not in d, k
    d2 = _run_stub("--steps", "6", "--warmup", "2", "--batch", "32", "--dump-outputs", str(tmp_path / "b"))
    assert d2["steps"] == 6
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["iters.npy", "status.npy", "u.npy", "x.npy"], names
    for n in names:
        a, a2 = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == 32, (n, a.dtype, a.shape)
        assert np.array_equal(a, a2), n
    # which step that was: the stub has 4 output sets (one per distinct batch) on 2 streams, so the warm-up runs max(2, 4) steps and the
    # timed steps start at the next multiple of 2 x 4 = 8: steps 8 .. 13, batch 8 % 4 = 0 first and batch 13 % 4 = 1 last
    u = np.load(tmp_path / "a" / "u.npy")
    from g1_locomotion_amd import synth
    feet = [synth.synthetic_batch(32, 10, seed=1000 + 97 * j, schedule="single")[2].reshape(32, 10, 12) for j in range(b.NBATCH)]
    first, last = 8 % b.NBATCH, (8 + 6 - 1) % b.NBATCH
    assert first != last and u.shape == (32, 10, 12)
    assert np.array_equal(u, feet[last]) and not np.array_equal(u, feet[first])
    assert np.all(np.load(tmp_path / "a" / "status.npy") == 1)
    # with the collective: the gathered forces are part of what the path returns
    d3 = _run_stub("--force-dist", "--steps", "3", "--warmup", "1", "--batch", "16", "--dump-outputs", str(tmp_path / "c"))
    assert d3["config"]["allgather_in_value"] is True and "value_without_allgather" not in d3
    assert np.array_equal(np.load(tmp_path / "c" / "u0_all.npy"), np.load(tmp_path / "c" / "u.npy")[:, 0, :])


def test_dump_outputs_keeps_a_seeded_sample_of_qps_within_its_budget(tmp_path):
    """Above the budget one seeded sample of QPs is kept in every array -- the rows of the same QPs, packed rows included -- and the
    files stay under the budget, the same from call to call."""
    import numpy as np
    b = _bench()
    rng = np.random.default_rng(1)
    B = 1000
    arrays = {"u": rng.random((B, 10, 12)), "x": rng.random((B, 11, 13)).astype(np.float32), "iters": rng.integers(1, 250, B).astype(np.int32)}
    total = sum(a.nbytes for a in arrays.values())
    assert b.dump_outputs(str(tmp_path / "all"), arrays, B) == 1.0
    assert np.array_equal(np.load(tmp_path / "all" / "iters.npy"), arrays["iters"].astype(np.float64))
    assert not (tmp_path / "all" / "qp_index.npy").exists()
    budget = total // 4
    for d in ("s1", "s2"):
        keep = b.dump_outputs(str(tmp_path / d), arrays, B, budget=budget)
        assert 0.2 < keep <= 0.25
    out = {k: np.load(tmp_path / "s1" / (k + ".npy")) for k in list(arrays) + ["qp_index"]}
    assert sum(out[k].nbytes for k in arrays) <= budget
    for k, a in out.items():
        assert np.array_equal(a, np.load(tmp_path / "s2" / (k + ".npy"))), k             # the same sample every time
    q = out["qp_index"].astype(np.int64)
    assert np.all(np.diff(q) > 0) and len(q) == out["u"].shape[0]
    for k in arrays:
        assert np.array_equal(out[k], arrays[k][q].astype(out[k].dtype)), k
    # a ragged fleet: u packed N_b rows per QP, x N_b + 1 rows per QP from row off_b + b, status one per QP (srbdqp.h)
    Nq = rng.choice([8, 12, 16, 24], size=B)
    off = np.concatenate([[0], np.cumsum(Nq)])
    ru, rx, st = rng.random((off[-1], 12)), rng.random((off[-1] + B, 13)), rng.integers(0, 3, B).astype(np.int32)
    rows_of = {"u": lambda q: np.concatenate([np.arange(off[i], off[i] + Nq[i]) for i in q]),
               "x": lambda q: np.concatenate([np.arange(off[i] + i, off[i] + i + Nq[i] + 1) for i in q])}
    budget = (ru.nbytes + rx.nbytes + st.nbytes) // 5
    b.dump_outputs(str(tmp_path / "r"), {"u": ru, "x": rx, "status": st}, B, rows_of, budget=budget)
    r = {k: np.load(tmp_path / "r" / (k + ".npy")) for k in ("u", "x", "status", "qp_index")}
    assert sum(r[k].nbytes for k in ("u", "x", "status")) <= budget
    q = r["qp_index"].astype(np.int64)
    assert np.array_equal(r["status"], st[q].astype(np.float64))
    assert np.array_equal(r["u"], np.concatenate([ru[off[i]:off[i] + Nq[i]] for i in q]))
    assert np.array_equal(r["x"], np.concatenate([rx[off[i] + i:off[i] + i + Nq[i] + 1] for i in q]))
