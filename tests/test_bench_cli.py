"""bench.py host logic that needs no GPU: the N > 1 self-launch (a CHILD torch.distributed.run,
started before torch or librau is imported -- never an exec from a process that touched the GPU)
and the strong-scaling argument handling."""
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_importing_bench_does_not_import_torch_or_load_librau():
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('b', 'bench.py'); "
            "m = u.module_from_spec(s); s.loader.exec_module(m); "
            "assert 'torch' not in sys.modules and 'rau_vqa_amd._lib' not in sys.modules")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_self_launch_starts_a_child_rendezvous_on_loopback(monkeypatch):
    b = load_bench()
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=7)

    monkeypatch.setattr(b.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--global-batch", "512"])
    with pytest.raises(SystemExit) as e:
        b.self_launch(types.SimpleNamespace(gpus=4))
    assert e.value.code == 7                                   # the child's code is relayed
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--global-batch", "512"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_rank_count_mismatch_and_indivisible_global_batch_are_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--global-batch", "7"], cwd=ROOT,
                       env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "not divisible" in r.stderr


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_writes_float32_within_the_budget(tmp_path):
    import numpy as np
    b = load_bench()
    rng = np.random.default_rng(0)
    arrays = {"logits": rng.standard_normal((4, 8, 50)).astype(np.float32),
              "argmax": np.arange(32, dtype=np.int32).reshape(4, 8),
              "grad_mult": rng.standard_normal(1000)}
    b.dump_outputs(str(tmp_path / "all"), arrays)
    for k, a in arrays.items():                    # under the budget: every array whole, shape kept
        got = np.load(tmp_path / "all" / f"{k}.npy")
        assert got.dtype == np.float32 and got.shape == a.shape
        np.testing.assert_array_equal(got, a.astype(np.float32))
    budget = 2000                                  # over it: the same seeded sample in every run
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    total = 0
    for k, a in arrays.items():
        s1, s2 = np.load(tmp_path / "s1" / f"{k}.npy"), np.load(tmp_path / "s2" / f"{k}.npy")
        np.testing.assert_array_equal(s1, s2)
        assert s1.dtype == np.float32 and 0 < s1.size < a.size
        assert np.all(np.isin(s1, a.astype(np.float32).ravel()))
        total += s1.nbytes
    assert total <= budget


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run prints the headline fields and nothing that --full measures; two runs with the
    same arguments dump the same outputs."""
    import json
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--batch", "16", "--dump-outputs", str(d)],
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        for k in ("roofline", "bulk_kernels", "step_incl_update_ms", "inference", "other_configs",
                  "cpu_baseline"):
            assert k not in line
        files = sorted(p.name for p in d.iterdir())
        assert {"losses.npy", "logits.npy", "argmax.npy", "grad_embed.npy", "grad_rnn.npy",
                "grad_mult.npy"} <= set(files)
        assert sum(p.stat().st_size for p in d.iterdir()) <= 64 * 10**6
        dumps.append({f: np.load(d / f) for f in files})
    assert dumps[0]["losses.npy"].shape == (8,)
    for f, a in dumps[0].items():
        assert a.dtype == np.float32 and np.all(np.isfinite(a)), f
        np.testing.assert_allclose(dumps[1][f], a, rtol=1e-5, atol=1e-7, err_msg=f)
