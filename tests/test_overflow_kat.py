"""Collision candidate tests with test-only builds (_build.TEST_VARIANTS), each bound to its own sims
(PickPlaceVecEnv(lib=...)) beside the product in this process.  The test builds compile both step kernels with
their defines, and every test with a test build runs on both layouts (Sim.step_rows: 128 rows, and the 192 rows
with a helper wave that small batches get).

* Contact-overflow KAT: more sphere-test survivors than the candidate list holds must reach
  env_error as ERR_CON_OVERFLOW, whichever substep of the env step overflowed (the flag is sticky from
  the record load to the step's fold).  The product list holds 320 of the 780 pairs, which no C3 state
  comes near, so the path is forced with libmmx_col4.so (a 4-entry list); the product library shows no
  overflow over a C3 rollout.
* The persistent broadphase list against the full prune (libmmx_nolist.so: a 1-entry list, so every
  pass runs the full prune): bit-identical states and contacts through the release / retreat phases.
* Two builds alive in one process do not mix: a product sim stepped in turn with a libmmx_col4.so sim computes
  what it computes alone, and only the col4 sim overflows."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def c3_env(n, lib, rows, autoreset=False):
    """n seeded C3 envs on the build `lib` (a path; None: the product) and the `rows` layout."""
    import oracle_py as O
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(n, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=autoreset, image_size=0, lib=lib)
    env.sim.step_rows = rows
    assert env.sim.step_rows == rows
    env.reset(seed=[O.episode_seed(42, i) for i in range(n)])
    return env


def state_digest(env) -> str:
    """SHA-256 of qpos, qvel and the last substep's contact record."""
    from mujoco_manip_amd import _lib

    h = hashlib.sha256()
    for t in (env.qpos, env.qvel, env.sim.view("contacts", _lib.MAXCON * _lib.CON_F)):
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def expert_steps(envs, steps=12):
    """`steps` expert env steps of every env of `envs`, in turn -> per env (digest, envs that overflowed, NaN envs)."""
    from mujoco_manip_amd import _lib

    hit = [np.zeros(e.num_envs, bool) for e in envs]
    for t in range(steps):
        for e, h in zip(envs, hit):
            e.step(e.expert_plan(16))
            h |= (e.env_error.cpu().numpy() & _lib.ERR_CON_OVERFLOW) != 0
    return [(state_digest(e), int(h.sum()), int(((e.env_error.cpu().numpy() & _lib.ERR_NAN) != 0).sum()))
            for e, h in zip(envs, hit)]


@pytest.mark.parametrize("rows", [128, 192])
def test_candidate_list_overflow_reaches_env_error(rows):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _build

    env = c3_env(64, _build.test_variant("libmmx_col4.so"), rows)
    (_, overflow, nan), = expert_steps([env])
    env.close()
    print("OVERFLOW_ENVS", overflow, "NAN_ENVS", nan)
    assert overflow > 0  # envs whose sphere test kept more than 4 pairs (3 cubes on the table + the gripper)


def test_product_c3_rollout_has_no_contact_overflow():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import oracle_py as O
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    n = 1024
    env = PickPlaceVecEnv(n, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          image_size=0)
    env.reset(seed=[O.episode_seed(42, i) for i in range(n)])
    seen = np.zeros(n, np.int32)
    for t in range(60):  # approach, grasps, transport: the contact piles
        env.step(env.expert_plan(16))
        seen |= env.env_error.cpu().numpy()
    env.close()
    assert not (seen & (_lib.ERR_CON_OVERFLOW | _lib.ERR_EFC_OVERFLOW)).any()


def block_digests(n, lib, rows):
    """Nine rollout_expert(10) blocks of n C3 envs with autoreset -> (digest after each, FSM states seen)."""
    env = c3_env(n, lib, rows, autoreset=True)
    out, phases = [], set()
    for k in range(9):
        env.rollout_expert(10)
        torch.cuda.synchronize()
        phases |= set(env.fsm_state.cpu().numpy().tolist())
        out.append(state_digest(env))
    env.close()
    return out, phases


@pytest.mark.parametrize("rows", [128, 192])
def test_broadphase_list_equals_full_prune(rows):
    """the persistent broadphase list (the pairs within 8 cm of contact when it was
    built, kept while the bodies' displacement bound stays under half of that) gives the same
    candidates, in the same order, as the full 780-pair prune.  512 C3 envs (256 on the 192-row layout: the
    smallest batch that still reaches the last phases) for 90 env steps (approach, grasp, transport,
    release, retreat): the product library (a 256-entry list) and the test build
    libmmx_nolist.so (a 1-entry list: the full prune in every collision pass) end every 10-step block
    with bit-identical states and last-substep contact lists."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _build

    n = 512 if rows == 128 else 256
    res = [block_digests(n, lib, rows) for lib in (_build.LIB, _build.test_variant("libmmx_nolist.so"))]
    print(sorted(res[0][1]), res[0][0][:3])
    assert {8, 9} <= res[0][1]  # release and retreat were reached
    assert res[0][0] == res[1][0]


@pytest.mark.parametrize("rows", [128, 192])
def test_two_libraries_alive_do_not_mix(rows):
    """Two builds of the same sources export the same functions and define kernels of the same names.  64 C3
    envs, 12 expert steps (the overflow test's shape): the product sim stepped in turn with a live
    libmmx_col4.so sim ends in the state it reaches alone, bit for bit; the col4 sim runs its own 4-entry
    list (it overflows), the product sim its own (it does not)."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _build

    env = c3_env(64, None, rows)
    (alone, overflow_alone, _), = expert_steps([env])
    env.close()
    envs = [c3_env(64, None, rows), c3_env(64, _build.test_variant("libmmx_col4.so"), rows)]
    assert envs[0].sim.L is not envs[1].sim.L
    (product, overflow_product, _), (_, overflow_col4, _) = expert_steps(envs)
    for e in envs:
        e.close()
    print("digest alone", alone, "beside col4", product, "overflow envs: product", overflow_product, "col4", overflow_col4)
    assert product == alone
    assert overflow_col4 > 0
    assert overflow_product == 0 and overflow_alone == 0
