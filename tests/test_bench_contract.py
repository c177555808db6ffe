"""bench.py launch contract (VERDICT r1 missing #3): `--gpus N` must never silently run one rank.
CPU tests: the launcher logic runs before torch is imported.  GPU test: two ranks rehearsed on one card (gloo)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE=1" in r.stderr and not r.stdout.strip()


def test_gpus_n_spawns_n_ranks_before_touching_the_gpu(monkeypatch):
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    had_cuda_init = "torch" in sys.modules and sys.modules["torch"].cuda.is_initialized()
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                      # the children's exit code is the bench's exit code
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index(BENCH) + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    if "torch" in sys.modules:
        assert sys.modules["torch"].cuda.is_initialized() == had_cuda_init


def _bench_module():
    sys.path.insert(0, ROOT)
    import importlib
    return importlib.import_module("bench")


def test_a_plain_run_leaves_the_secondary_legs_to_full():
    bench = _bench_module()
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(["--full", "--no-extra", "--dump-outputs", "out"])
    assert a.full and a.no_extra and not a.no_cpu_baseline and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_writes_the_last_step_as_float_npy(tmp_path, monkeypatch):
    """CPU stand-in for a training workload: the step's loss, the logged terms and the gradients; an array above
    DUMP_SAMPLE elements is written as the same seeded sample in every run."""
    import numpy as np
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)

    class Wl:
        pass
    wl = Wl()
    torch.manual_seed(0)
    wl.model = torch.nn.Sequential(torch.nn.Linear(8, 4), torch.nn.Linear(4, 2)).train()
    loss = wl.model(torch.randn(3, 8)).pow(2).mean()
    loss.backward()
    wl.tb = {"loss_cls": loss.detach() * 0.5, "n_pos": 3, "note": "text is not an array"}
    wl.opt = Wl()
    wl.opt.exp_avg, wl.opt.exp_avg_sq = torch.linspace(-1, 1, 48), torch.linspace(0, 2, 48)
    for d in ("a", "b"):
        bench.dump_outputs(wl, loss.detach(), str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["adam_exp_avg.npy", "adam_exp_avg_sq.npy", "gradients.npy", "loss.npy", "tb_loss_cls.npy",
                     "tb_n_pos.npy"]
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert got["loss.npy"].dtype == np.float32 and float(got["loss.npy"]) == float(loss.detach())
    assert got["tb_n_pos.npy"].dtype == np.float64 and float(got["tb_n_pos.npy"]) == 3.0
    grads = torch.cat([p.grad.reshape(-1) for p in wl.model.parameters()]).numpy()
    assert grads.size == 46 and np.array_equal(got["gradients.npy"], grads)
    assert np.array_equal(got["adam_exp_avg_sq.npy"], wl.opt.exp_avg_sq.numpy())
    big = torch.arange(1000, dtype=torch.float64)
    bench.dump_outputs(Wl(), big, str(tmp_path / "c"))
    bench.dump_outputs(Wl(), big, str(tmp_path / "d"))
    c, d = np.load(tmp_path / "c" / "output.npy"), np.load(tmp_path / "d" / "output.npy")
    assert c.dtype == np.float64 and c.size == 50 and np.array_equal(c, d) and (np.diff(c) > 0).all()


def test_training_workloads_restart_every_step_from_the_state_of_construction():
    """TrainStepWorkload.restore (bench.time_workload calls it before every step) writes the first snapshot back in place."""
    import torch
    sys.path.insert(0, ROOT)
    from benchmarks import workloads
    from pdanet_amd import _lib, optimization

    class Wl:
        restore = workloads.TrainStepWorkload.restore
    wl = Wl()
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(8, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))
    wl.opt = optimization.build_optimizer(model, workloads.TrainStepWorkload.OPTIM)
    p0 = wl.opt.flat_p.clone()
    ptr, epoch = wl.opt.flat_p.data_ptr(), _lib.WEIGHT_EPOCH[0]
    wl.restore()                                           # first call: the snapshot
    with torch.no_grad():                                  # what an optimizer step does
        wl.opt.flat_p.add_(0.5)
        wl.opt.exp_avg.fill_(1.0)
        wl.opt.exp_avg_sq.fill_(2.0)
    wl.opt.step_count = 7
    wl.restore()
    assert torch.equal(wl.opt.flat_p, p0) and wl.opt.flat_p.data_ptr() == ptr
    assert not wl.opt.exp_avg.any() and not wl.opt.exp_avg_sq.any() and wl.opt.step_count == 0
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in model[0].parameters()]), p0[:36])   # views of flat_p
    assert _lib.WEIGHT_EPOCH[0] >= epoch + 2


def _run_bench(env, argv, limit=150, attempts=2):
    """bench.py in its own session, killed as a process group at `limit` seconds (torch.distributed.run's workers are
    grandchildren).  One of ~25 two-rank one-card rehearsals of round 3 stopped making progress for minutes and was never
    reproduced; the stacks of every thread are dumped before the kill (PDA_DUMP_STACKS_AFTER) and the
    run is repeated once, so a one-off stall is reported in the test output instead of costing the whole suite its time limit."""
    import signal
    env = dict(env, PDA_DUMP_STACKS_AFTER=str(limit - 20))
    last = None
    for attempt in range(attempts):
        p = subprocess.Popen([sys.executable, BENCH] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             start_new_session=True)
        try:
            out, err = p.communicate(timeout=limit)
            return subprocess.CompletedProcess(p.args, p.returncode, out, err)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            out, err = p.communicate()
            last = (out, err)
            print("bench.py %s: no result after %d s (attempt %d); stderr tail:\n%s" % (argv, limit, attempt + 1, err[-3000:]))
    raise AssertionError("bench.py stalled %d times; last stderr tail: %s" % (attempts, last[1][-2000:]))


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["0", "1"])
def test_two_ranks_on_one_card_report_world_size_2(tail):
    """The whole --gpus 2 path of bench.py (self-spawn -> torch.distributed.run -> flat-buffer gradient all-reduce -> MAX
    over ranks -> one JSON line) with both ranks on the one GPU of the box over gloo (RCCL refuses two ranks per device).
    The ranks run the SAME graphed step as a single rank: head + losses (tail = 0) or layers 3-5 + head + losses (tail = 1)
    replayed as hipGraphs, the gradient exchange outside every captured region (round 2 crashed here under DDP)."""
    env = dict(os.environ, PDA_REHEARSE_ONE_GPU="1", PDA_DIST_BACKEND="gloo", PDA_GRAPH_TAIL=tail, PYTHONFAULTHANDLER="1")
    env.pop("WORLD_SIZE", None)
    env.pop("PDA_GRAPH_HEAD", None)
    env.pop("PDA_DDP", None)
    r = _run_bench(env, ["--gpus", "2", "--steps", "3", "--warmup", "1", "--points", "4096", "--no-cpu-baseline", "--no-extra"])
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world_size_seen"] == 2 and d["config"]["global_batch"] == 4
    assert "flat fp32 gradient buffer" in d["config"]["gradient_exchange"] and d["value"] > 0 and d["scaling"] == "weak"
    assert d["config"]["graph_head"] is True and d["config"]["graph_tail"] is (tail == "1")


@pytest.mark.gpu
def test_two_ranks_reference_shaped_ddp_path():
    """PDA_DDP=1 keeps the reference's DistributedDataParallel wrapper (tools/train.py:153-154) available: eager head."""
    env = dict(os.environ, PDA_REHEARSE_ONE_GPU="1", PDA_DIST_BACKEND="gloo", PDA_DDP="1", PYTHONFAULTHANDLER="1")
    env.pop("WORLD_SIZE", None)
    r = _run_bench(env, ["--gpus", "2", "--steps", "2", "--warmup", "0", "--points", "4096", "--no-cpu-baseline", "--no-extra"])
    assert r.returncode == 0, r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and "DistributedDataParallel" in d["config"]["gradient_exchange"]
    assert d["config"]["graph_head"] is False and d["config"]["graph_tail"] is False


@pytest.mark.gpu
def test_a_training_loop_that_keeps_its_loss_survives_the_late_tail_capture():
    """`loss = wl.step()` in a loop keeps the previous iteration's return value alive while the next one runs.  The KITTI
    workload captures its tail graph on the fifth iteration (the host-bound probe runs on the fourth); with the autograd graph
    of the fourth iteration alive through that loss, the capture died inside hipStreamEndCapture (DESIGN.md "Known gaps").
    The workloads return the loss detached: the loop below -- in its own process, a crash there is a signal, not an
    exception -- must come through, with the tail graphed."""
    code = ("import sys, torch; sys.path.insert(0, %r)\n"
            "from benchmarks import workloads as bw\n"
            "wl = bw.create('kitti_detector_train', 4, 16384, torch.device('cuda:0'), 0, 1); wl.begin()\n"
            "for i in range(8):\n"
            "    l = wl.step()\n"
            "torch.cuda.synchronize()\n"
            "assert not l.requires_grad and l.grad_fn is None\n"
            "print('graph_tail', wl.model.graph_tail, float(l))\n" % ROOT)
    env = dict(os.environ, PDA_GRAPH_TAIL="auto", PYTHONFAULTHANDLER="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "graph_tail" in r.stdout


@pytest.mark.gpu
def test_a_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """The plain line carries the headline fields and nothing of --full; --dump-outputs writes the last timed step, and two
    runs with the same arguments write the same outputs: the forward pass's loss terms to the last bits, the gradients and
    the Adam moments the optimizer kernels wrote from them to the rounding of one backward pass (float-atomic sums)."""
    import numpy as np
    env = dict(os.environ, PYTHONFAULTHANDLER="1")
    env.pop("WORLD_SIZE", None)
    runs = []
    for k in range(2):
        out = tmp_path / ("outputs%d" % k)
        r = _run_bench(env, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--points", "4096", "--dump-outputs", str(out)],
                       attempts=1)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "scenes/s" and d["higher_is_better"] is True
        assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert d["config"]["full"] is False and d["roofline"] is None
        assert not {"cpu_baseline", "cpu_baseline_ops", "extra", "roofline_ball_query"} & set(d)
        arrays = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
        assert {"loss", "gradients", "adam_exp_avg", "adam_exp_avg_sq"} <= set(arrays)
        assert any(n.startswith("tb_") for n in arrays)
        assert np.abs(arrays["adam_exp_avg"]).max() > 0 and arrays["adam_exp_avg_sq"].min() >= 0
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        runs.append(arrays)
    a, b = runs
    assert sorted(a) == sorted(b)
    for n in a:
        if n == "loss" or n.startswith("tb_"):
            assert np.allclose(a[n], b[n], rtol=1e-5, atol=0), (n, a[n], b[n])
        else:
            scale = float(np.abs(a[n]).max())
            assert np.allclose(a[n], b[n], rtol=1e-4, atol=1e-5 * scale), (n, float(np.abs(a[n] - b[n]).max()), scale)
