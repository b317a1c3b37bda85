"""The rollout plan's launch count, restated for the tests (csrc/mmx_plan.h rollout_plan, without cameras);
shared by tests/test_gpu.py (against a live sim) and tests/test_host_selftest.py (against the host program)."""


def plan_launches(n, fuse, lanes):
    """mmx_rollout_expert's plan (mmx_plan.h rollout_plan): len = min(fuse, ceil(n / 4)); lane l starts
    with l * len / lanes steps, then launches of len, then the remainder; the most launches of a lane."""
    ln = max(1, min(fuse, -(-n // 4)))
    out = 0
    for l in range(lanes):
        first = min(n, l * ln // lanes)
        out = max(out, (1 if first else 0) + -(-(n - first) // ln))
    return out
