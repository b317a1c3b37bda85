"""bench.py's command line: the plain run (one timed window, nothing beyond the headline figure) and
--dump-outputs (the env's output buffers after the last timed step, float32 .npy files).

GPU: one small plain run in a fresh process with --dump-outputs; the dumped arrays are bit-equal to
the buffers of an in-process env driven through the same seeded reset / warm-up / timed rollout.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP = 48, 16, 4


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd.shard import shard_seeds
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--envs-per-gpu", str(N), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    # one window of exactly --steps env steps; ms_per_step is that window's time per step
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["repeats"]["n"] == 1
    assert line["ms_per_step"] > 0
    np.testing.assert_allclose(line["value"], N * 1000.0 / line["ms_per_step"], rtol=1e-9)
    assert line["solver"]["substeps"] == N * STEPS * 16  # the window ran STEPS env steps, no more
    assert line["cpu_baseline"] is None and line["render"] is None  # --full's legs stayed off

    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          image_size=0, autoreset=True)
    env.reset(seed=shard_seeds(42, 0, 1, N))
    env.rollout_expert(WARMUP)
    env.rollout_expert(STEPS)
    torch.cuda.synchronize()
    want = {"obs": env._obs, "reward": env._reward, "done": env._done, "reward_components": env._rc,
            "qpos": env.qpos, "qvel": env.qvel, "ctrl": env.ctrl}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    total = 0
    for k, t in want.items():
        got = np.load(out / (k + ".npy"))
        assert got.dtype == np.float32 and got.shape == tuple(t.shape), k
        np.testing.assert_array_equal(got, t.cpu().numpy().astype(np.float32), err_msg=k)
        total += got.nbytes
    assert total <= 64 << 20
    assert np.abs(np.load(out / "obs.npy")).max() > 0
