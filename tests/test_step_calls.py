"""What the env-step kernel carries across its out-of-line calls (step_begin, 16 x substep, step_finish).
Those functions are compiled without callee-saved registers (mmx_step_kernels.inc, MMX_NO_TAIL_MARK), so the
kernel itself keeps its live values over every call: the env index read from the dispatch order, the step
and substep counters, and the contact destination handed to the last substep only.  A value lost over a
call shows as another env's record, a substep too many or too few, or a contact record that is missing or
written after the wrong substep.

48 C3 envs, seeded, 8 expert env steps, run six ways:
  fused     one rollout_expert(8): two env steps per launch, the plan made inside the kernel
  stepwise  eight expert_plan -> step calls: one env step per launch, the action read from memory
  prof      one rollout_expert(8) on libmmx_prof.so (the phase-clock build: it also keeps the per-phase
            snapshot, the FSM state and two clocks live across the 16 substep calls), bound to its own sims
each on the 128-row and the 192-row layout.  qpos, qvel, ctrl, observation, reward, done flags and the
last substep's contact record are bit-identical across all six."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ENVS, N_STEPS, SEED = 48, 8, 42
FIELDS = ("qpos", "qvel", "ctrl", "obs", "reward", "done", "contacts")


def collect(rows: int, fused: bool, lib=None) -> dict:
    """One run on the build `lib` of the library (a path; None: the product): field -> SHA-256 of its bytes
    after the 8 env steps, plus the number of contacts in the record ("ncon") and the envs with an error bit
    ("err")."""
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(N_ENVS, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True, image_size=0, lib=lib)
    env.sim.step_rows = rows
    assert env.sim.step_rows == rows
    env.reset(seed=SEED)
    if fused:
        assert env.sim.rollout_launches(N_STEPS) < N_STEPS  # more than one env step per launch
        env.rollout_expert(N_STEPS)
    else:
        for _ in range(N_STEPS):
            env.step(env.expert_plan(16))
    torch.cuda.synchronize()
    arrays = {"qpos": env.qpos, "qvel": env.qvel, "ctrl": env.ctrl, "obs": env._obs, "reward": env._reward,
              "done": env._done, "contacts": env.sim.view("contacts", _lib.MAXCON * _lib.CON_F)}
    out = {k: hashlib.sha256(arrays[k].contiguous().cpu().numpy().tobytes()).hexdigest()[:16] for k in FIELDS}
    out["ncon"] = int(env._epi[:, _lib.EPI["ncon"]].sum().item())
    out["err"] = int((env.env_error != 0).sum().item())
    env.close()
    return out


_RUNS: dict = {}


def _runs():
    """The six runs, once for the module: name -> collect()'s result."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _build

    if not _RUNS:
        for rows in (128, 192):
            _RUNS[f"fused{rows}"] = collect(rows, True)
            _RUNS[f"stepwise{rows}"] = collect(rows, False)
            _RUNS[f"prof{rows}"] = collect(rows, True, _build.test_variant("libmmx_prof.so"))
        for name, d in _RUNS.items():
            print(name, d)
    return _RUNS


def test_rollout_reaches_contacts_without_errors():
    """The inputs are worth comparing: every run's last substep wrote contacts (the cubes rest on the
    table) and no env carries an error bit."""
    for name, d in _runs().items():
        assert d["ncon"] > 0, name
        assert d["err"] == 0, name


@pytest.mark.parametrize("field", FIELDS)
def test_six_runs_bit_identical(field):
    runs = _runs()
    digests = {name: d[field] for name, d in runs.items()}
    assert len(digests) == 6
    assert len(set(digests.values())) == 1, digests
