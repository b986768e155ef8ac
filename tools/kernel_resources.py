#!/usr/bin/env python
"""Per-kernel register / scratch / LDS usage of the HIP extension, from hipcc's -Rpass-analysis=kernel-resource-usage.

  python tools/kernel_resources.py [substring ...]     (cross-compiles for gfx950; no GPU needed)

Instruction counts of the build's own assembly, for the kernels whose demangled name holds one of the substrings:

  python tools/kernel_resources.py --isa [--unit qip_tile_interp] [--blocks] k_tile_passes

prints one histogram line per kernel (f64 / f32 multiplies and adds, v_mov_b64 + v_mov_b32, v_cndmask, LDS instructions, scalar
loads, branches) and the instructions of the gate loop's latch: the block that advances the descriptor pointer by
sizeof(TileGate), which every gate executes ("latch"), and separately each copy-only block that falls through into it ("in
front": the tail of whichever cases jump there, with the number of branches that do).  --blocks adds one line per basic block (the same counts and where it branches to), which
is what the executed path of one gate kind is read from.  Every unit is compiled with the options rustqip_amd/build.py gives it."""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_UNITS = ("qip_launch", "qip_circuit", "qip_tile_interp", "qip_slice", "qip_host", "qip_measure", "qip_pauli", "qip_function", "qip_multiplex", "qip_qft", "qip_channel", "qip_dist")  # the units that launch kernels


def build_flags():
    spec = importlib.util.spec_from_file_location("_qip_build", os.path.join(ROOT, "rustqip_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, mod.FLAGS, mod.UNIT_FLAGS


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return out[: len(names)]
    except FileNotFoundError:
        return names


CLASSES = (("mul64", r"v_mul_f64"), ("add64", r"v_add_f64"), ("mul32", r"v_mul_f32"), ("add32", r"v_(add|sub|subrev)_f32"),
           ("mov", r"v_mov_b(64|32)"), ("cnd", r"v_cndmask"), ("ds", r"ds_"), ("sload", r"s_(buffer_)?load"),
           ("branch", r"s_c?branch"))
GATE_BYTES = (0x80, 0x40)  # sizeof(TileWireGate<double>), sizeof(TileWireGate<float>): what the interpreter's gate loop advances by


def count(lines):
    h = dict.fromkeys([c for c, _ in CLASSES], 0)
    for ln in lines:
        op = ln.split()[0]
        for c, pat in CLASSES:
            if re.match(pat, op):
                h[c] += 1
                break
    return h


def fmt(h):
    return " ".join("%s %4d" % (c, h[c]) for c, _ in CLASSES)


def functions(path):
    """{mangled name: [(block label, [instruction, ...]), ...]} of one assembly file"""
    out, cur, blocks = {}, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur, blocks = m.group(1), [("entry", [])]
            out[cur] = blocks
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", ln) or re.match(r"^; %(bb\.\d+):", ln)
        if m:
            blocks.append((m.group(1), []))
            continue
        t = ln.strip()
        if not t or t[0] in ";." or t.startswith("s_nop") or t.startswith("s_waitcnt"):
            continue
        blocks[-1][1].append(t.split(";")[0].rstrip())
    return out


def latch(blocks):
    """indices of the blocks that fall through into the pointer advance, and of that block"""
    for i, (_, ins) in enumerate(blocks):
        if any(re.match(r"s_add_u32 (s\d+), \1, (0x%x|%d)$" % (b, b), x) for x in ins for b in GATE_BYTES):  # (the assembler prints 64 in decimal)
            j = i
            while j > 0 and blocks[j - 1][1] and not re.match(r"s_branch|s_endpgm|s_setpc", blocks[j - 1][1][-1]) and \
                    all(re.match(r"v_mov|v_accvgpr", x) for x in blocks[j - 1][1]):
                j -= 1
            return list(range(j, i + 1))
    return []


def isa_mode(args):
    hipcc, flags, unit_flags = build_flags()
    units = [args[i + 1] for i, a in enumerate(args) if a == "--unit"] or list(KERNEL_UNITS)
    skip = {i + 1 for i, a in enumerate(args) if a == "--unit"}
    want = [a for i, a in enumerate(args) if not a.startswith("--") and i not in skip]
    for unit in units:
        asm = "/tmp/qip_isa_%s.s" % unit
        if "--cached" not in args or not os.path.exists(asm):
            cmd = [hipcc, *[f for f in flags if f != "-fPIC"], *unit_flags.get(unit, []), "--cuda-device-only", "-S", "-o", asm,
                   os.path.join(ROOT, "rustqip_amd", "csrc", unit + ".hip")]
            subprocess.run(cmd, stderr=subprocess.DEVNULL, check=True)
        fns = functions(asm)
        for name, nm in zip(fns, demangle(list(fns))):
            if want and not any(w in nm for w in want):
                continue
            blocks = fns[name]
            print("%s\n  all      %s" % (nm[:150], fmt(count([x for _, ins in blocks for x in ins]))))
            lt = latch(blocks)
            if lt:
                # the block that advances the descriptor pointer is the latch proper: every gate executes it.  The copy-only
                # blocks in front of it fall through into it, but a gate executes one only if its case jumps there: "entered by"
                # counts the branches of the whole kernel that do (0 = reached only by falling through from the block above)
                targets = [x.split()[-1] for _, ins in blocks for x in ins if re.match(r"s_c?branch", x)]
                for i in lt:
                    kind = "latch   " if i == lt[-1] else "in front"
                    print("  %s %s  %s: entered by %d branches" % (kind, fmt(count(blocks[i][1])), blocks[i][0], targets.count(blocks[i][0])))
                    for x in blocks[i][1]:
                        print("        " + x)
            if "--blocks" in args:
                for lab, ins in blocks:
                    to = [x.split()[-1] for x in ins if re.match(r"s_c?branch", x)]
                    print("  %-10s %s  -> %s" % (lab, fmt(count(ins)), " ".join(to)))


def main():
    if "--isa" in sys.argv:
        return isa_mode(sys.argv[1:])
    hipcc, flags, unit_flags = build_flags()
    res = "/tmp/qip_kernel_resources.txt"
    if not (len(sys.argv) > 1 and sys.argv[1] == "--cached" and os.path.exists(res)):
        with open(res, "w") as f:
            for unit in KERNEL_UNITS:
                cmd = [hipcc, *flags, *unit_flags.get(unit, []), "-c", "-o", "/tmp/qip_res.o", os.path.join(ROOT, "rustqip_amd", "csrc", unit + ".hip"),
                       "-Rpass-analysis=kernel-resource-usage"]
                subprocess.run(cmd, stderr=f, check=True)
    want = [a for a in sys.argv[1:] if not a.startswith("--")]
    txt = open(res).read()
    blocks = re.split(r"remark: [^\n]*Function Name: ", txt)[1:]
    rows = []
    for b in blocks:
        def g(k):
            m = re.search(k + r": (\d+)", b)
            return int(m.group(1)) if m else -1
        rows.append((b.split("\n")[0].strip(), g("VGPRs"), g("AGPRs"), g("SGPRs"), g(r"ScratchSize \[bytes/lane\]"),
                     g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")))
    names = demangle([r[0] for r in rows])
    print("vgpr agpr sgpr scratch occ lds  kernel")
    for r, nm in zip(rows, names):
        if not want or any(w in nm for w in want):
            print("%4d %4d %4d %6d %3d %5d  %s" % (r[1], r[2], r[3], r[4], r[5], r[6], nm[:160]))


if __name__ == "__main__":
    main()
