"""tools/isa_same.py on two small synthetic listings: functions that are equal up to local labels, branch
targets, pc-relative literals, function order and end padding give exit status 0; one changed operand
gives a non-zero status and names the function."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a hipcc -S listing: a device function and a kernel that calls it
LISTING_A = """\t.text
\t.type\t_Z4stepi,@function
_Z4stepi:                               ; @_Z4stepi
; %bb.0:
\ts_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0)
\tv_cmp_gt_i32_e32 vcc, 1, v0
\ts_cbranch_vccnz .LBB0_2
; %bb.1:
\tv_add_u32_e32 v0, 3, v0
.LBB0_2:
\ts_setpc_b64 s[30:31]
.Lfunc_end0:
\t.size\t_Z4stepi, .Lfunc_end0-_Z4stepi
\t.globl\tkern
\t.type\tkern,@function
kern:                                   ; @kern
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_getpc_b64 s[2:3]
\ts_add_u32 s2, s2, _Z4stepi@rel32@lo+4
\ts_addc_u32 s3, s3, _Z4stepi@rel32@hi+12
\ts_swappc_b64 s[30:31], s[2:3]
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel kern
\t.end_amdhsa_kernel
\t.text
.Lfunc_end1:
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .name: kern
...
\t.end_amdgpu_metadata
"""

# the same two functions in the other order, with other label numbers, another distance to the callee
# (a data symbol before it) and the padding of an object's last kernel
LISTING_B = """\t.text
\t.globl\tkern
\t.type\tkern,@function
kern:                                   ; @kern
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_getpc_b64 s[2:3]
\ts_add_u32 s2, s2, _Z4stepi@rel32@lo+20
\ts_addc_u32 s3, s3, _Z4stepi@rel32@hi+28
\ts_swappc_b64 s[30:31], s[2:3]
\ts_endpgm
.Lfunc_end0:
\t.type\t_Z4stepi,@function
_Z4stepi:                               ; @_Z4stepi
\ts_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0)
\tv_cmp_gt_i32_e32 vcc, 1, v0
\ts_cbranch_vccnz .LBB1_7
\tv_add_u32_e32 v0, 3, v0
.LBB1_7:
\ts_setpc_b64 s[30:31]
\ts_nop 0
\ts_nop 0
.Lfunc_end1:
"""

# two llvm-objdump -d outputs of the kernel at different addresses
OBJDUMP_A = """
Disassembly of section .text:

0000000000001900 <kern>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001900: C0060002 00000000
\ts_getpc_b64 s[2:3]                                         // 000000001908: BE821C00
\ts_add_u32 s2, s2, 0x1f4                                    // 00000000190C: 8002FF02 000001F4
\ts_addc_u32 s3, s3, 0                                       // 000000001914: 82038003
\ts_cbranch_scc1 65533                                       // 000000001918: BF85FFFD <kern+0x10>
\ts_endpgm                                                   // 00000000191C: BF810000
"""
OBJDUMP_B = OBJDUMP_A.replace("0x1f4", "0x2a8").replace("000001F4", "000002A8").replace("65533", "12").replace("19", "2a")


def run(tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    return subprocess.run([sys.executable, os.path.join(REPO, "tools", "isa_same.py"), str(pa), str(pb), "-v"],
                          capture_output=True, text=True, timeout=60)


def test_equal_up_to_labels_order_and_padding(tmp_path):
    r = run(tmp_path, LISTING_A, LISTING_B)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "equal: kern (6)" in r.stdout and "equal: _Z4stepi (5)" in r.stdout
    assert "2 / 2 functions, 11 / 11 instructions, 0 differ" in r.stdout
    r = run(tmp_path, OBJDUMP_A, OBJDUMP_B)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1 / 1 functions, 6 / 6 instructions, 0 differ" in r.stdout


def test_one_changed_operand_is_found(tmp_path):
    r = run(tmp_path, LISTING_A, LISTING_B.replace("v_add_u32_e32 v0, 3, v0", "v_add_u32_e32 v0, 4, v0"))
    assert r.returncode != 0
    assert "DIFFERS: _Z4stepi" in r.stdout and "equal: kern" in r.stdout and "1 differ" in r.stdout
    # a literal that is not pc-relative is not masked; a missing function counts
    r = run(tmp_path, OBJDUMP_A, OBJDUMP_A.replace("s[4:5], 0x0", "s[4:5], 0x8"))
    assert r.returncode != 0 and "DIFFERS: kern" in r.stdout
    r = run(tmp_path, LISTING_A, LISTING_B.replace("_Z4stepi:", "_Z5stepxi:"))
    assert r.returncode != 0 and "ONLY IN first: _Z4stepi" in r.stdout
