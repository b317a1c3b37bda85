"""The GJK pair class's cache of separating axes (csrc/mmx_gjk_cache.h; convex_convex in csrc/mmx_geom.h) on the
GPU, both step layouts: no result depends on it, and it is taken.

1 Cache on equals cache off: the product and the build without the cache (libmmx_nocache.so) run nine
  rollout_expert(10) blocks of seeded C3 envs with autoreset (512 envs at 128 rows, 256 at 192: the smallest
  batches that reach release and retreat, as tests/test_overflow_kat.py's list test found); states and
  last-substep contact records are bit-identical after every block.
2 Cold, warm and stale caches: the near-miss scenes (gaps 4e-5 to 9e-5 m) and the 5e-5 m penetrating rung of
  the narrowphase sweep's GJK classes (every class with a hull or a cylinder that is no floor pair), one env
  each, one substep through the physics harness.  A sim steps the scenes from the same state twice (the second
  time its entries are those the first left), then with every env given another scene (the next one, and the
  one six further: the same class's other kind), so the entries are another state's; each time the contact
  records, the contact counts and the stepped state equal a fresh sim's, bit for bit.
3 The cache is taken: on the build with probe set 15 (libmmx_gjkprobe.so: GJK calls, separated calls,
  support-query rounds and cached verdicts in the stats) the near-miss scenes, stepped from the same state
  again and again (a persistent separated candidate), show no cached verdict in the first substep and at least
  one per env in every later one; a cached verdict is one round where the uncached call took at least two, and
  an env whose only GJK candidate is the near miss runs exactly one round.  libmmx_nocache.so shows none.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWEEP = json.load(open(os.path.join(GOLDEN, "narrowphase_sweep.json")))
# the classes the GJK / EPA pass takes: a hull (mesh) or a leg (cylinder) on either side, and no plane
GJK_CLASSES = [c for c, groups in SWEEP["classes"].items()
               if c not in SWEEP["uncovered"] and any(g in ("hull", "leg") for g in groups[0]) and "floor" not in groups[0]]
MISS = [s for s in SWEEP["scenes"] if s["cls"] in GJK_CLASSES and s["kind"] == "miss"]
HIT = [s for s in SWEEP["scenes"] if s["cls"] in GJK_CLASSES and s["kind"] == "hit" and s["rung"] == 5e-5]


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# --------------------------------------------------------------------------- 1: cache on equals cache off
def block_digests(n, lib, rows):
    """Nine rollout_expert(10) blocks of n seeded C3 envs with autoreset on the build `lib` (None: the product)
    -> (SHA-256 of qpos, qvel and the last substep's contact record after each block, FSM states seen)."""
    import oracle_py as O
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(n, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True, image_size=0, lib=lib)
    env.sim.step_rows = rows
    assert env.sim.step_rows == rows
    env.reset(seed=[O.episode_seed(42, i) for i in range(n)])
    out, phases = [], set()
    for k in range(9):
        env.rollout_expert(10)
        torch.cuda.synchronize()
        phases |= set(env.fsm_state.cpu().numpy().tolist())
        h = hashlib.sha256()
        for t in (env.qpos, env.qvel, env.sim.view("contacts", _lib.MAXCON * _lib.CON_F)):
            h.update(t.cpu().numpy().tobytes())
        out.append(h.hexdigest()[:16])
    env.close()
    return out, phases


@pytest.mark.parametrize("rows", [128, 192])
def test_cache_on_equals_cache_off(rows):
    need_gpu()
    from mujoco_manip_amd import _build

    n = 512 if rows == 128 else 256
    on, phases = block_digests(n, None, rows)
    off, _ = block_digests(n, _build.test_variant("libmmx_nocache.so"), rows)
    print(sorted(phases), on[:3])
    assert {8, 9} <= phases  # release and retreat were reached
    assert on == off


# --------------------------------------------------------------------------- 2: cold, warm and stale caches
class Harness:
    """One env per scene on one sim; step(Q): the scenes' states loaded, one substep, everything it left."""

    def __init__(self, n, rows, lib=None):
        from mujoco_manip_amd import _lib

        self.L = _lib
        self.sim = _lib.Sim(n, action_mode="abs_pos", image_size=0, lib=lib)
        self.sim.reset()
        self.sim.step_rows = rows
        assert self.sim.step_rows == rows
        self.ctrl = self.sim.get_state()[2]
        self.n = n

    def step(self, Q):
        L, n = self.L, self.n
        self.sim.set_state(Q, np.zeros((n, 27), np.float32), self.ctrl, np.zeros((n, 27), np.float32))
        self.sim.physics_step(1, with_ik=False)
        epi = self.sim.view("episode_i", L.EPI_N, "<i4").cpu().numpy()
        qpos, qvel, _, _ = self.sim.get_state()
        return dict(con=self.sim.view("contacts", L.MAXCON * L.CON_F).cpu().numpy().copy(),
                    ncon=epi[:, L.EPI["ncon"]].copy(), err=epi[:, L.EPI["env_error"]].copy(), qpos=qpos, qvel=qvel)

    def stats(self):
        return self.sim.view("stats", self.L.STAT_N).double().cpu().numpy().copy()

    def close(self):
        self.sim.close()


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)


@pytest.mark.parametrize("rows", [128, 192])
def test_cold_warm_and_stale_caches_change_nothing(rows):
    need_gpu()
    scenes = []
    for c in GJK_CLASSES:  # per class its near misses, then its shallowest hits
        scenes += [s for s in MISS if s["cls"] == c] + [s for s in HIT if s["cls"] == c]
    assert len(GJK_CLASSES) == 8 and all(sum(1 for s in MISS if s["cls"] == c) >= 6 for c in GJK_CLASSES)
    Q = np.array([s["qpos"] for s in scenes], np.float32)
    n = len(scenes)
    fresh = {}
    for shift in (0, 1, 6):  # a fresh sim per arrangement: nothing in its caches but zeros
        h = Harness(n, rows)
        fresh[shift] = h.step(np.roll(Q, -shift, axis=0))
        h.close()
    is_miss = np.array([s["kind"] == "miss" for s in scenes])
    back = fresh[0]
    assert (back["ncon"] > 0).any() and not (back["err"] != 0).any()
    h = Harness(n, rows)
    cold = h.step(Q)
    warm = h.step(Q)
    stale1 = h.step(np.roll(Q, -1, axis=0))
    stale6 = h.step(np.roll(Q, -6, axis=0))
    again = h.step(Q)  # and back: entries of the shifted scenes
    h.close()
    assert same(cold, fresh[0]), "cold"
    assert same(warm, fresh[0]), "warm"
    assert same(stale1, fresh[1]), "stale (the next scene)"
    assert same(stale6, fresh[6]), "stale (the class's other kind)"
    assert same(again, fresh[0]), "stale (back)"
    # the scenes are what the test is about: a miss env and the env of its class's hit differ in their contacts
    assert is_miss.sum() >= 48 and (~is_miss).sum() >= 48


# --------------------------------------------------------------------------- 3: the cache is taken
AUX = slice(13, 17)  # STAT_T_AUX0..3: calls, separated, rounds, cached verdicts (probe set 15)


def probe_steps(lib, rows, steps=4):
    Q = np.array([s["qpos"] for s in MISS], np.float32)
    h = Harness(len(MISS), rows, lib)
    prev, out = h.stats()[:, AUX], []
    for k in range(steps):
        h.step(Q)
        now = h.stats()[:, AUX]
        out.append(now - prev)
        prev = now
    h.close()
    return out


@pytest.mark.parametrize("rows", [128, 192])
def test_the_cache_is_taken(rows):
    need_gpu()
    from mujoco_manip_amd import _build, _lib

    assert _lib.STAT_N > 16
    on = probe_steps(_build.test_variant("libmmx_gjkprobe.so"), rows)
    off = probe_steps(_build.test_variant("libmmx_nocache.so"), rows)
    first = on[0]
    calls, sep, rounds, cached = first.T
    print("first substep: calls", calls.sum(), "separated", sep.sum(), "rounds", rounds.sum(), "cached", cached.sum())
    assert (calls >= 1).all() and (sep >= 1).all()  # every scene's near miss is a GJK candidate, and ends separated
    assert (cached == 0).all() and (rounds >= 2 * calls).all()  # uncached: the start round and at least one more
    single = (calls == 1) & (sep == 1)
    assert single.sum() >= 6, single.sum()
    for k, d in enumerate(on[1:], 2):
        c2, s2, r2, h2 = d.T
        print("substep", k, "calls", c2.sum(), "separated", s2.sum(), "rounds", r2.sum(), "cached", h2.sum())
        assert (c2 == calls).all() and (s2 == sep).all()  # the same candidates, the same verdicts
        assert (h2 >= 1).all()  # a cached verdict in every env, from the second substep on
        assert (r2 <= rounds - h2).all()  # each replaced at least two rounds by one
        assert (r2[single] == 1).all() and (h2[single] == 1).all()  # the near miss alone: one round
    for d in off:
        assert (d[:, 3] == 0).all() and np.array_equal(d, off[0])  # compiled out: no verdict, every substep the same
    assert np.array_equal(off[0][:, :3], first[:, :3])  # and what the product's first, uncached substep did
