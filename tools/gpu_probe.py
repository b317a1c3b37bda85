"""GPU-vs-oracle diagnostic probe (writes gpurun_out/probe.json). Test infrastructure."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import oracle_py as O  # noqa: E402
import torch  # noqa: E402

from mujoco_manip_amd import _lib  # noqa: E402

out = {}


def states_from_oracle_rollout(n_states=32, seed=0):
    """Collect diverse states (free space, resting, grasping, transporting) from an oracle FSM episode."""
    e = O.OracleEnv()
    e.reset_keyframe()
    e.fsm_init([(0, 0)])
    states = []
    k = 0
    while len(states) < 200 and k < 2000:
        e.fsm_plan(16)
        e.fsm_actuate()
        for _ in range(16):
            e.mj_step()
        states.append(e.get_state())
        k += 1
        if e.fsm_get()["state"] == 10:
            break
    idx = np.linspace(0, len(states) - 1, n_states).astype(int)
    return [states[i] for i in idx]


def physics_parity(n_sub):
    sts = states_from_oracle_rollout(64)
    N = len(sts)
    sim = _lib.Sim(N)
    qpos = np.stack([s[0] for s in sts], 0).astype(np.float32)
    qvel = np.stack([s[1] for s in sts], 0).astype(np.float32)
    ctrl = np.stack([s[2] for s in sts], 0).astype(np.float32)
    ws = np.stack([s[3] for s in sts], 0).astype(np.float32)
    sim.set_state(qpos, qvel, ctrl, ws)
    sim.physics_step(n_sub, with_ik=False)
    gq, gv, _, _ = sim.get_state()
    dq, dv, nefc_o = [], [], []
    for k, s in enumerate(sts):
        e = O.OracleEnv()
        e.set_state(qpos[k].astype(float), qvel[k].astype(float), ctrl[k].astype(float), ws[k].astype(float))
        for _ in range(n_sub):
            e.mj_step()
        rq, rv, _, _ = e.get_state()
        dq.append(np.abs(gq[k] - rq).max())
        dv.append(np.abs(gv[k] - rv).max())
        nefc_o.append(e.nefc())
    st = sim.view("stats", _lib.STAT_N).double().cpu().numpy()
    epi = sim.view("episode_i", _lib.EPI_N, "<i4").cpu().numpy()
    return {"max_dqpos": float(max(dq)), "max_dqvel": float(max(dv)), "per_state_dq": [float(x) for x in dq],
            "per_state_dv": [float(x) for x in dv], "mean_nefc": float(st[:, 0].sum() / max(st[:, 3].sum(), 1)),
            "nefc_gpu_last": epi[:, 11].tolist(), "nefc_oracle_last": nefc_o,
            "mean_solver_iter": float(st[:, 2].sum() / max(st[:, 3].sum(), 1)), "max_resid": float(st[:, 4].max())}


def gym_parity(steps=30, mode="abs_pos"):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    N = 8
    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True)
    obs, _ = env.reset(seed=100)
    refs = [O.OracleEnv(action_mode="abs_pos", reward_type="staged", randomize_objects=True) for _ in range(N)]
    robs = np.stack([r.reset(seed=100 + k) for k, r in enumerate(refs)])
    flat = lambda o: torch.cat([o[k].reshape(N, -1) for k in o], 1).cpu().numpy()  # noqa: E731
    d0 = np.abs(flat(obs) - robs).max(0)
    tasks_match = [tuple(refs[k].task()) for k in range(N)] == [(int(a), int(b)) for a, b in zip(env._epi[:, 0].cpu(), env._epi[:, 1].cpu())]
    errs = []
    for t in range(steps):
        act = env.expert_plan(16)
        obs, r, term, trunc, info = env.step(act)
        a = act.cpu().numpy()
        ro = np.stack([refs[k].step(a[k])[0] for k in range(N)])
        errs.append(float(np.abs(flat(obs)[:, :11] - ro[:, :11]).max()))
    return {"reset_obs_maxdiff_per_field": d0.tolist(), "tasks_match": bool(tasks_match), "step_state_err": errs}


def expert_success(N=256, steps=150):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True)
    env.reset(seed=0)
    t = time.time()
    placed = torch.zeros(N, dtype=torch.bool, device="cuda")
    done_at = torch.full((N,), -1, device="cuda")
    for k in range(steps):
        act = env.expert_plan(16)
        obs, r, term, trunc, info = env.step(act)
        placed |= (env.episode_flags & 8) != 0
        fsm_done = env.fsm_state == 10
        done_at = torch.where((done_at < 0) & fsm_done, torch.full_like(done_at, k), done_at)
    torch.cuda.synchronize()
    return {"placed_rate": float(placed.float().mean()), "fsm_done_rate": float((done_at >= 0).float().mean()),
            "mean_done_step": float(done_at[done_at >= 0].float().mean()) if (done_at >= 0).any() else -1,
            "env_error": int((env.env_error != 0).sum()),
            "env_error_bits": {str(b): int(((env.env_error & b) != 0).sum()) for b in (1, 2, 4, 8)},
            "secs": time.time() - t, "solver": env.solver_stats()}


def rollout_speed(N=4096, steps=100, warm=50):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True, image_size=int(os.environ.get("MMX_IMAGE_SIZE", "0")))
    env.reset(seed=[_lib.episode_seed(42, i) for i in range(N)])
    env.rollout_expert(warm)  # bench-like state mix (50 warm-up steps)
    torch.cuda.synchronize()
    env.clear_stats()
    t = time.time()
    env.rollout_expert(steps)
    torch.cuda.synchronize()
    dt = time.time() - t
    return {"env_steps_per_s": N * steps / dt, "ms_per_step": 1000 * dt / steps, "solver": env.solver_stats()}


FSM_NAMES = ("idle", "pre_grasp", "grasp", "close_gripper", "lift", "move_to_bin", "settle_at_bin", "lower_to_bin",
             "release", "retreat", "done")


def fsm_profile(N=4096, steps=160, warm=0):
    """Diagnostic (profiling) build: per FSM state of the C3 rollout, env steps, mean shader cycles
    per env step (whole step and per phase), solver iterations / rows / contacts per substep.
    Cycles are one wave's wall time in shader clocks (two waves share a SIMD)."""
    import ctypes as C

    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    L = _lib.load()
    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True)
    env.reset(seed=[_lib.episode_seed(42, i) for i in range(N)])
    if warm:
        env.rollout_expert(warm)
    torch.cuda.synchronize()
    nf = L.mmx_fsm_profile_fields()
    buf = (C.c_double * (11 * nf))()
    L.mmx_fsm_profile.argtypes = [C.POINTER(C.c_double), C.c_int]
    L.mmx_fsm_profile(buf, 1)
    env.rollout_expert(steps)
    torch.cuda.synchronize()
    L.mmx_fsm_profile(buf, 1)
    a = np.array(buf[:]).reshape(11, nf)
    phases = ["ik", "kinematics", "dynamics", "collision", "constraints", "solver", "integrate", "step_end", "aux0",
              "aux1", "aux2", "aux3"]
    P = len(phases)
    out = {"probe_set": os.environ.get("MMX_LIB_PATH", "libmmx_prof.so")}
    tot = a[:, nf - 1].sum()
    for s in range(11):
        n = a[s, nf - 1]
        if n == 0:
            continue
        out[FSM_NAMES[s]] = {"env_steps": int(n), "share": n / tot, "cycles_per_env_step": a[s, P] / n,
                             **{p + "_per_substep": a[s, j] / (16 * n) for j, p in enumerate(phases) if p != "step_end"},
                             "step_end": a[s, 7] / n,
                             "solver_iter_per_substep": a[s, P + 1] / (16 * n),
                             "nefc_per_substep": a[s, P + 2] / (16 * n),
                             "ncon_per_substep": a[s, P + 3] / (16 * n)}
    allc = (a[:, P]).sum() / tot
    # shader clock over the env steps: s_memtime cycles / s_memrealtime seconds (100 MHz ticks)
    out["all"] = {"env_steps": int(tot), "cycles_per_env_step": allc,
                  "shader_clock_ghz": float(a[:, P].sum() / max(a[:, nf - 2].sum(), 1.0) * 0.1)}
    return out


def nefc_dist(N=4096, steps=400):
    """Probe set 12 build: max nefc / ncon per env over a C3 rollout, substeps with nefc > 192 / 224."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True)
    env.reset(seed=[_lib.episode_seed(42, i) for i in range(N)])
    env.clear_stats()
    env.rollout_expert(steps)
    torch.cuda.synchronize()
    st = env.sim.view("stats", _lib.STAT_N).double().cpu().numpy()
    sub = st[:, 3].sum()
    mx = st[:, 13]
    return {"substeps": float(sub), "max_nefc": float(mx.max()), "p999_env_max_nefc": float(np.quantile(mx, 0.999)),
            "p99_env_max_nefc": float(np.quantile(mx, 0.99)), "max_ncon": float(st[:, 14].max()),
            "frac_nefc_gt192": float(st[:, 15].sum() / sub), "frac_nefc_gt224": float(st[:, 16].sum() / sub),
            "mean_nefc": float(st[:, 0].sum() / sub),
            "efc_overflow_envs": int(((env.env_error & 2) != 0).sum()) if hasattr(env, "env_error") else -1}


def gjk_dist(N=4096, steps=160):
    """Probe set 16 build: the most GJK candidates any env had in one collision pass of a C3 rollout (the size of
    the axis cache's table, csrc/mmx_gjk_cache.h), and the share of passes with more than 2, 4 and
    MMX_AXIS_SLOTS of them."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True)
    env.reset(seed=[_lib.episode_seed(42, i) for i in range(N)])
    env.clear_stats()
    env.rollout_expert(steps)
    torch.cuda.synchronize()
    st = env.sim.view("stats", _lib.STAT_N).double().cpu().numpy()
    sub = st[:, 3].sum()
    return {"substeps": float(sub), "max_gjk_candidates": float(st[:, 13].max()),
            "p999_env_max": float(np.quantile(st[:, 13], 0.999)), "frac_gt2": float(st[:, 14].sum() / sub),
            "frac_gt4": float(st[:, 15].sum() / sub), "frac_gt_slots": float(st[:, 16].sum() / sub)}


def digest(N=2048, steps=160):
    """Bit-identity digest of a C3 expert rollout: sha256 of qpos / qvel / obs after every 20 steps
    (A/B of two builds that must agree bit for bit)."""
    import hashlib

    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True)
    env.reset(seed=[_lib.episode_seed(42, i) for i in range(N)])
    out = []
    for k in range(steps // 20):
        env.rollout_expert(20)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        h.update(env.qpos.cpu().numpy().tobytes())
        h.update(env.qvel.cpu().numpy().tobytes())
        out.append(h.hexdigest()[:16])
    return {"digests": out, "ncon": float(env.sim.view("stats", _lib.STAT_N).double()[:, 1].sum().item())}


if __name__ == "__main__":
    os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
    for name, fn in [("phys1", lambda: physics_parity(1)), ("phys16", lambda: physics_parity(16)),
                     ("gym", gym_parity), ("expert", expert_success), ("speed", rollout_speed),
                     ("nefc", nefc_dist), ("gjk", gjk_dist), ("fsm", fsm_profile), ("digest", digest)]:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        t = time.time()
        try:
            out[name] = fn()
        except Exception as ex:  # keep going: this is a probe
            import traceback

            out[name] = {"error": repr(ex), "tb": traceback.format_exc()}
        out[name + "_secs"] = time.time() - t
        print(name, json.dumps(out[name])[:600], flush=True)
        with open(os.path.join(REPO, "gpurun_out", "probe_prof.json" if os.environ.get("MMX_PROFILE", "0") not in ("", "0") else "probe.json"), "w") as f:
            json.dump(out, f, indent=1)
