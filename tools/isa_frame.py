"""Scratch frames and spill instructions of the step kernel's functions in a hipcc -S listing: the
evidence behind the HBM traffic of the out-of-line substep.  Usage:
    hipcc ... --cuda-device-only -S mmx_kernels.hip -o k.s ; python tools/isa_frame.py k.s [k2.s]
(mmx_kernels.hip holds the 128-row step kernels through mmx_step.inc and its mmx_step_*.inc parts,
mmx_step_l192.hip the 192-row ones.)
Per function: private segment bytes per lane, VGPRs, scratch stores / loads (the callee-saved save
area and spills), v_writelane / v_readlane (SGPR spills into VGPR lanes and cross-lane reads).
functions() is the listing splitter, shared with tools/isa_same.py."""
import collections
import re
import sys

FUNCS = ("_Z7substepifPf", "mmx_env_step_kernel", "mmx_env_step_budget_kernel", "mmx_env_step_kernel_l192",
         "_Z10step_beginRK8MMXStateiPKfii",
         "_Z11step_finishRK8MMXStatei", "mmx_env_traj_kernel", "mmx_env_traj_kernel_l192",
         "_Z10policy_actRK8MMXStateRK9MmxPolicyRK12MMXPolicyRecij", "mmx_env_policy_kernel",
         "mmx_env_policy_kernel_l192", "_Z17dagger_policy_actRK8MMXStateRK9MmxPolicyRK12MMXPolicyRecij",
         "_Z12dagger_beginRK8MMXStateRK9MmxPolicyRK9MMXDaggerij", "mmx_env_dagger_kernel",
         "mmx_env_dagger_kernel_l192")  # (a listing holds one layout's kernels: the other's are left out)

# a function's label: `name:` in a -S listing, `0000000000001900 <name>:` in llvm-objdump -d output
LABEL = re.compile(r"^(?:[0-9a-f]+ <)?([A-Za-z_][\w.$]*)>?:\s*(;.*)?$")


def functions(txt):
    """(function, line) for every non-empty line below a function's label, local labels included."""
    fn, in_text = None, True
    for line in txt.split("\n"):
        d = line.split()[0] if line.strip() else ""
        if d in (".section", ".amdgpu_metadata", ".text", ".data", ".bss", ".rodata"):  # data sections and notes are no function's lines
            in_text = d == ".text" or (d == ".section" and ".text" in line)
            continue
        m = LABEL.match(line)
        if m and in_text and not m.group(1).startswith((".L", "$")):
            fn = m.group(1)
            continue
        if fn and in_text and line.strip():
            yield fn, line


def frames(path):
    txt = open(path).read()
    ops = collections.defaultdict(collections.Counter)
    for fn, line in functions(txt):
        t = line.strip().split()
        for k in ("scratch_store", "scratch_load", "v_writelane", "v_readlane"):
            if t[0].startswith(k):
                ops[fn][k] += 1
    out = {}
    for f in FUNCS:
        seg = re.search(rf"\.set (?:\.L)?{re.escape(f)}\.private_seg_size, (\d+)(\+max)?", txt)
        if not seg and f.startswith(("_Z10policy_act", "_Z17dagger_policy_act", "_Z12dagger_begin")):
            continue  # (a listing of before the policy kernel, or the DAgger kernel)
        vg = re.search(rf"\.set (?:\.L)?{re.escape(f)}\.num_vgpr, (?:max\()?(\d+)", txt)
        if f.startswith("mmx_env_") and not seg:
            continue
        out[f] = {"private_seg_bytes_per_lane": int(seg.group(1)) if seg else None,
                  "plus_callees": bool(seg and seg.group(2)), "vgpr": int(vg.group(1)) if vg else None, **ops[f]}
    return out


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print(p)
        for f, d in frames(p).items():
            print(f"  {f[:34]:34s} {d}")
