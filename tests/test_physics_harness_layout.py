"""mmx_physics_step runs the one-substep kernel of the layout the sim is set to (mmx_set_step_rows): the
128-row single-wave kernel, or the 192-row kernel with its helper wave.  Every physics-level known-answer
and parity test goes through Sim.physics_step, so which kernel it launches decides what those tests cover.

The evidence is the phase clock of the profile build (libmmx_prof.so, which build() makes), loaded in a
child process because the binding holds one library per process: in the 128-row kernel the env's wave runs
the dynamics itself and clocks it (cyc_dynamics > 0); in the helper layout the dynamics run on the helper
wave beside the broadphase and the env wave never clocks that phase (cyc_dynamics stays 0), while the
kinematics and the solver are clocked in both."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import sys
import numpy as np
import torch
assert torch.cuda.is_available()
sys.path.insert(0, sys.argv[1])
from mujoco_manip_amd import _lib
rows = int(sys.argv[2])
sim = _lib.Sim(2, action_mode="abs_pos", image_size=0)
sim.reset()
sim.step_rows = rows
assert sim.step_rows == rows
cols = [_lib.STAT_FIELDS.index(k) for k in ("cyc_ik", "cyc_kinematics", "cyc_dynamics", "cyc_solver", "substeps")]
before = sim.view("stats", _lib.STAT_N).cpu().numpy()[:, cols].astype(float)
sim.physics_step(1, with_ik=True)
after = sim.view("stats", _lib.STAT_N).cpu().numpy()[:, cols].astype(float)
err = sim.view("episode_i", _lib.EPI_N, "<i4")[:, _lib.EPI["env_error"]].cpu().numpy()
assert (err == 0).all(), err
assert np.isfinite(sim.get_state()[0]).all()
for e in range(2):
    print("CLOCKS", e, " ".join(repr(float(x)) for x in after[e] - before[e]))
sim.close()
"""


@pytest.mark.parametrize("rows", [128, 192])
def test_physics_step_runs_the_sims_layout(rows):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    lib = os.path.join(REPO, "mujoco_manip_amd", "libmmx_prof.so")
    assert os.path.exists(lib), "profile build missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if k != "MMX_STEP_ROWS"}
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, str(rows)], env=dict(env, MMX_LIB_PATH=lib),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("CLOCKS")]
    assert len(lines) == 2, r.stdout
    for ln in lines:
        ik, kin, dyn, solve, substeps = map(float, ln)
        print(f"rows={rows} cyc_ik={ik} cyc_kinematics={kin} cyc_dynamics={dyn} cyc_solver={solve}")
        assert substeps == 1.0 and kin > 0 and solve > 0, ln
        if rows == 128:
            assert dyn > 0 and ik > 0, ln
        else:
            assert dyn == 0, ln
