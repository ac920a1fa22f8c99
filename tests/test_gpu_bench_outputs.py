"""bench.py --dump-outputs on the GPU: a plain run (no --full) of T timed steps writes what its
last call returned; the state and the carried key must equal the CPU oracle's rollout of the same
T steps from the reset state (so --steps sets the timed steps and the dump is the timed run's), the
last step's rewards and dones the oracle's, and the line keeps its headline keys while the --full
measurements stay out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.data.windows import make_windows
from hftlob.layout import pack_env_cfg
from oracle import pyoracle as O
from test_gpu_env import _float_words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_steps_outputs(tmp_path):
    E, T, N_MSGS = 200, 5, 30_000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", str(E), "--steps", str(T),
           "--warmup", "2", "--n-msgs", str(N_MSGS), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == T and line["value"] > 0 and line["unit"] == "env steps/s" and line["dtype"] == "int32"
    assert line["higher_is_better"] is True and "env steps/sec" in line["metric"]
    assert abs(line["ms_per_step"] - E * 1e3 / line["value"]) <= 1e-4 + 1e-3 * line["ms_per_step"]
    assert line["unsettled"] is None and line["episode_value"] is None and line["cpu_baseline"] is None

    cfg = builtin_config("2_player_fq_fqc")
    w = cfg.world_config
    day = generate_day(n_msgs=N_MSGS, mid=2_000_000, snap_every=w.n_data_msg_per_step * w.start_resolution)
    win = make_windows(day, w)
    c, L = pack_env_cfg(cfg, len(win.starts), day.msgs.shape[0], True)
    init = O.init_states(c.lob, win, day.msgs, w, L.init_rec_words)
    keys = O.split_keys(np.zeros((1, 2), np.uint32), E + 1)[0]
    st, _ = O.env_reset(c, keys[1:], init)
    master = keys[0].copy()
    for _ in range(T):
        ks = O.split_keys(master[None], E + 1)[0]
        master, sk = ks[0].copy(), ks[1:].copy()
        st, _, rew, done_all, dones, _ = O.env_step(c, sk, O.sample_actions(c, sk), day.msgs, init, st)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["env_rows"].tolist() == list(range(E))
    fw = _float_words(type("E", (), {"layout": L})()).tolist()
    iw =[j for j in range(L.rec_words) if j not in fw]
    assert (got["state_int"] == st[:, iw]).all()
    assert np.allclose(got["state_float"], st[:, fw].view(np.float32), rtol=1e-5, atol=1e-5)
    assert (got["carried_key"] == master).all()
    n_types = len(cfg.number_of_agents_per_type)
    assert np.allclose(np.concatenate([got[f"rewards_type{t}"].reshape(E, -1) for t in range(n_types)], 1),
                       np.asarray(rew).reshape(E, -1), rtol=1e-5, atol=1e-5)
    assert (np.concatenate([got[f"dones_type{t}"].reshape(E, -1) for t in range(n_types)], 1)
            == np.asarray(dones).reshape(E, -1)).all()
    assert (got["done_all"] == np.asarray(done_all).reshape(E)).all()
    assert all(got[f"obs_type{t}"].shape[0] == E and np.isfinite(got[f"obs_type{t}"]).all() for t in range(n_types))
