"""bench.py's multi-GPU entry point on the CPU: `--gpus N` outside torchrun starts N rank
processes itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set before anything touches the GPU);
`--dry-run` stops each rank before the GPU (gloo) and rank 0 prints the layout.  The ranks own
contiguous, disjoint env blocks of ONE Speed_test rollout over N * E envs (the reference's pmap
layout, ippo_rnn_JAXMARL_pmap.py:292-332)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True,
                       env=env, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_gpus_n_launches_n_ranks(n):
    E = 4096
    out = _run("--gpus", str(n), "--dry-run")
    assert out["dry_run"] and out["n_gpus"] == n and out["num_envs_total"] == n * E
    ranks = out["ranks"]
    assert [r["rank"] for r in ranks] == list(range(n))
    # contiguous, disjoint, covering [0, n*E); reset keys are rows 1.. of split(PRNGKey(0), n*E + 1)
    assert [r["envs"] for r in ranks] == [[i * E, (i + 1) * E] for i in range(n)]
    assert [r["reset_key_rows"] for r in ranks] == [[1 + i * E, 1 + (i + 1) * E] for i in range(n)]
    assert all(r["key_e0"] == r["envs"][0] and r["key_n"] == n * E for r in ranks)


def test_failing_rank_fails_the_launch():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--envs", "x"],
                       capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode != 0


def test_plain_run_is_the_default():
    """--full is off unless asked for; the episode window and the CPU baseline hang on it."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.parametrize("limit,world", [(64_000_000, 1), (300_000, 1), (300_000, 2)])
def test_dump_outputs_files(limit, world, tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 .npy files of what the last call returned, the int and the
    float words of the state record apart; over the size limit every per-env array keeps the same
    seeded rows (env_rows), the same on every call."""
    import types

    import numpy as np
    import torch

    import bench
    from hftlob.config_io import builtin_config
    from hftlob.layout import pack_env_cfg
    monkeypatch.setattr(bench, "DUMP_BYTES", limit)
    _, L = pack_env_cfg(builtin_config("2_player_fq_fqc"), 4, 10_000, True)
    E, g = 37, torch.Generator().manual_seed(1)
    buf = torch.randint(-2**31, 2**31 - 1, (E, L.rec_words), dtype=torch.int32, generator=g)
    fw = bench.float_words(L)
    buf[:, fw] = torch.rand((E, len(fw)), generator=g).view(torch.int32)
    obs = [torch.rand((E, 1, d), generator=g) for d in L.obs_dims]
    rew = [torch.rand((E, 1), generator=g) for _ in L.obs_dims]
    dones = {"__all__": torch.rand(E, generator=g) < 0.5, "agents": [torch.rand((E, 1), generator=g) < 0.5
                                                                    for _ in L.obs_dims]}
    ret = (obs, types.SimpleNamespace(buf=buf), rew, dones, None)
    env = types.SimpleNamespace(layout=L)
    key = torch.tensor([-5, 7], dtype=torch.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), env, ret, key, 0, world)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert set(got) == {"env_rows", "carried_key", "state_int", "state_float", "done_all", "obs_type0", "obs_type1",
                        "rewards_type0", "rewards_type1", "dones_type0", "dones_type1"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit // world
    rows = got["env_rows"].astype(np.int64)
    assert (np.diff(rows) > 0).all() and rows.min() >= 0 and rows.max() < E
    assert len(rows) == E if limit > 10**6 else 0 < len(rows) < E
    b = buf.numpy()
    iw = [j for j in range(L.rec_words) if j not in fw]
    assert (got["state_int"] == b[rows][:, iw]).all() and got["state_int"].dtype == np.float64
    assert (got["state_float"] == b[rows][:, fw].view(np.float32)).all()
    assert (got["obs_type1"] == obs[1].numpy()[rows]).all() and (got["rewards_type0"] == rew[0].numpy()[rows]).all()
    assert (got["done_all"] == dones["__all__"].numpy()[rows]).all()
    assert got["carried_key"].tolist() == [2**32 - 5, 7]
    for n, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (n + ".npy")))


def test_timed_window():
    """config.timed_window: the driver's 20-step window from the reset state never reaches the
    64-step episode's end (marl_env.py:711-718 fires at step counter 62); 128 steps cross two."""
    import bench
    assert "no episode end" in bench.timed_window(20, 64)
    assert "at timed step(s) [62, 125]" in bench.timed_window(128, 64)
    assert "at timed step(s) [62]" in bench.timed_window(63, 64)
    assert "no episode end" in bench.timed_window(62, 64)
