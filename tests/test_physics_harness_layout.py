"""mmx_physics_step runs the one-substep kernel of the layout the sim is set to (mmx_set_step_rows): the
128-row single-wave kernel, or the 192-row kernel with its helper wave.  Every physics-level known-answer
and parity test goes through Sim.physics_step, so which kernel it launches decides what those tests cover.

The evidence is the phase clock of the profile build (libmmx_prof.so, which build() makes), bound to the
test's sim (Sim(lib=...)): in the 128-row kernel the env's wave runs the dynamics itself and clocks it
(cyc_dynamics > 0); in the helper layout the dynamics run on the helper wave beside the broadphase and the
env wave never clocks that phase (cyc_dynamics stays 0), while the kinematics and the solver are clocked in
both."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def substep_clocks(rows, lib):
    """One physics substep of 2 envs on the build `lib`, `rows` layout -> per env the increase of (cyc_ik,
    cyc_kinematics, cyc_dynamics, cyc_solver, substeps)."""
    from mujoco_manip_amd import _lib

    sim = _lib.Sim(2, action_mode="abs_pos", image_size=0, lib=lib)
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
    sim.close()
    return after - before


@pytest.mark.parametrize("rows", [128, 192])
def test_physics_step_runs_the_sims_layout(rows, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _build

    monkeypatch.delenv("MMX_STEP_ROWS", raising=False)
    clocks = substep_clocks(rows, _build.test_variant("libmmx_prof.so"))
    assert len(clocks) == 2
    for ln in clocks.tolist():
        ik, kin, dyn, solve, substeps = ln
        print(f"rows={rows} cyc_ik={ik} cyc_kinematics={kin} cyc_dynamics={dyn} cyc_solver={solve}")
        assert substeps == 1.0 and kin > 0 and solve > 0, ln
        if rows == 128:
            assert dyn > 0 and ik > 0, ln
        else:
            assert dyn == 0, ln
