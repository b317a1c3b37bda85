"""Are two builds' functions the same instructions?  Compares two hipcc -S listings, or two
`llvm-objdump -d` outputs, of a device code object, function by function (isa_frame.functions splits
them): the way to show that a change which only moves or renames source left the kernels alone.  Usage:
    hipcc <the build's flags> --cuda-device-only -S mmx_kernels.hip -o new.s     (and the same before the change)
    python tools/isa_same.py old.s new.s [-v]
Before comparing, what depends on where a function lies is masked: local labels, branch targets and
pc-relative literals (`sym@rel32@lo+4`; in a disassembly the literal added to an s_getpc_b64 result);
comments, directives and the s_nop / s_code_end padding behind a function's last instruction are dropped.
Prints each function's verdict (-v: equal ones too) and the function and instruction counts; exit status 1
when a function differs or exists in one listing only (2 when a file holds no function at all).  The order
of the functions may differ."""
import re
import sys

from isa_frame import functions

MASKS = ((re.compile(r"\.L\w+"), "<L>"),
         (re.compile(r"[\w.$]+@(?:rel32|gotpcrel32)@(?:lo|hi)(?:[+-]\d+)?"), "<pcrel>"))
PCREL_OPS = ("s_add_u32", "s_addc_u32", "s_sub_u32", "s_subb_u32")
PADDING = ("s_nop 0", "s_code_end")


def instructions(txt):
    """{function: [masked instruction, ...]} of a listing or disassembly."""
    out, since_getpc = {}, {}
    for fn, line in functions(txt):
        s = " ".join(re.split(r";|//", line, maxsplit=1)[0].split())
        if not s or s.startswith(".") or s.endswith(":"):
            continue  # comment, directive or local label
        for rx, to in MASKS:
            s = rx.sub(to, s)
        op = s.split()[0]
        if op.startswith(("s_branch", "s_cbranch")):
            s = op + " <target>"
        elif op == "s_getpc_b64":
            since_getpc[fn] = 0
        elif op in PCREL_OPS and since_getpc.get(fn, 9) < 4:
            s = re.sub(r"\b0x[0-9a-f]+$", "<pcrel>", s)
        since_getpc[fn] = since_getpc.get(fn, 9) + 1
        out.setdefault(fn, []).append(s)
    for seq in out.values():
        while seq and seq[-1] in PADDING:
            seq.pop()
    return {f: seq for f, seq in out.items() if seq}


def compare(a_txt, b_txt, verbose=False, out=sys.stdout):
    a, b = instructions(a_txt), instructions(b_txt)
    if not a or not b:
        print("no function found in " + ("the first" if not a else "the second") + " file", file=out)
        return 2
    bad = 0
    for f in sorted(set(a) | set(b)):
        if f not in a or f not in b:
            print(f"ONLY IN {'first' if f in a else 'second'}: {f}", file=out)
            bad += 1
        elif a[f] != b[f]:
            k = next((i for i, (x, y) in enumerate(zip(a[f], b[f])) if x != y), min(len(a[f]), len(b[f])))
            print(f"DIFFERS: {f} ({len(a[f])} / {len(b[f])} instructions), first at {k}: "
                  f"{a[f][k] if k < len(a[f]) else '-'} | {b[f][k] if k < len(b[f]) else '-'}", file=out)
            bad += 1
        elif verbose:
            print(f"equal: {f} ({len(a[f])})", file=out)
    print(f"{len(a)} / {len(b)} functions, {sum(map(len, a.values()))} / {sum(map(len, b.values()))} instructions, "
          f"{bad} differ", file=out)
    return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "-v"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(compare(open(args[0]).read(), open(args[1]).read(), verbose="-v" in sys.argv))
