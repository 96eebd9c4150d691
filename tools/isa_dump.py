"""Per-kernel gfx950 disassembly of the built device objects (build/obj/<name>.o for every name in OBJECTS;
ISA_OBJDIR selects a variant build's objects).

    python tools/isa_dump.py OUTDIR            # one OUTDIR/<kernel>.s per kernel symbol
    python tools/isa_dump.py --diff DIR_A DIR_B
    python tools/isa_dump.py --regs [FILTER]   # kernel, VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes (tab-separated)

Used to show that a source change which should not alter the generated code (e.g. deleting
compile-time knobs at their default values) leaves every kernel's instructions identical.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


OBJECTS = ("kernels", "fused_odd", "narrow", "wide", "influence", "theta", "cluster", "fe_hip", "fe2_hip",
           "gee_hip")


def _code_objects(run):
    """run(name, path of the unbundled gfx950 code object) for every built device object."""
    objdir = os.environ.get("ISA_OBJDIR", os.path.join(ROOT, "build", "obj"))  # e.g. build/obj_<variant>
    for name in OBJECTS:
        obj = os.path.join(objdir, f"{name}.o")
        if not os.path.exists(obj):
            continue
        with tempfile.TemporaryDirectory() as d:
            fat, co = os.path.join(d, "fatbin"), os.path.join(d, "dev.co")
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.devnull],
                           check=True, capture_output=True)
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True,
                           capture_output=True)
            run(name, co)


def regs(flt: str = "") -> int:
    """The register / scratch / LDS figures of every kernel from the code objects' metadata notes."""
    rows = []

    def one(name, co):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            get = lambda k: (re.search(rf"\.{k}:\s*(\S+)", blk) or [None, "?"])[1]
            sym = get("name")
            filt = shutil.which("c++filt")  # mangled names where no demangler is installed
            dem = subprocess.run([filt, sym], capture_output=True, text=True).stdout.strip() if filt else sym
            # (only a template's name carries its return type)
            dem = re.sub(r"^(void )?sglm::(\(anonymous namespace\)::)?", "", dem).split("(")[0]
            rows.append((dem, get("vgpr_count"), blk.split()[0], get("sgpr_count"), get("private_segment_fixed_size"),
                         get("group_segment_fixed_size")))

    _code_objects(one)
    for r in sorted(rows):
        if flt in r[0]:
            print("\t".join(r))
    return len(rows)


def dump(outdir: str) -> int:
    os.makedirs(outdir, exist_ok=True)
    count = 0
    texts = []
    _code_objects(lambda name, co: texts.append(subprocess.run(
        [os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
        capture_output=True, text=True).stdout))
    for text in texts:
        cur, lines = None, []
        for line in text.splitlines():
            m = re.match(r"^(\S+):$", line.strip()) if line and not line.startswith((" ", "\t")) else None
            if m:
                if cur:
                    _write(outdir, cur, lines)
                    count += 1
                cur, lines = m.group(1), []
            elif cur and line.strip():
                # branch targets print as absolute addresses + symbol offsets: keep only the opcode/operands
                lines.append(re.sub(r"\s*//.*$", "", line.strip()))
        if cur:
            _write(outdir, cur, lines)
            count += 1
    return count


def _write(outdir, sym, lines):
    with open(os.path.join(outdir, sym[:200] + ".s"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _normalise(text: str):
    """A symbol's instructions without what only its place in the code object decides: the padding after its
    end (s_nop / s_code_end) and the PC-relative offsets of its calls and constant addresses (the two adds
    after an s_getpc_b64)."""
    lines = text.splitlines()
    while lines and re.match(r"(s_nop 0|s_code_end|\.\.\.|v_illegal.*)$", lines[-1]):
        lines.pop()
    out, pc = [], 0
    for ln in lines:
        if ln.startswith("s_getpc_b64"):
            pc = 2
        elif pc and re.match(r"s_addc?_u32 s\d+, s\d+, 0x[0-9a-f]+$", ln):
            ln = re.sub(r"0x[0-9a-f]+$", "PCREL", ln)
            pc -= 1
        out.append(ln)
    return out


def _kernarg_only(la, lb):
    """The (old, new) literal pairs if the only differences are offsets into the kernel-argument segment (a struct
    that grew at its end moves the hidden arguments behind it), else None.  Such a difference is a scalar load
    whose offset literal changed, or an `s_add_u32 sN, sM, literal` that forms the address of such an argument:
    the add counts only if its literal pair is one a scalar load of the same symbol shows or moves by the same
    amount as one, or if it adds to / from the low register of a pair the symbol's scalar loads use as their
    base (the segment pointer) -- a changed scalar constant of any other kind is an instruction difference."""
    if len(la) != len(lb):
        return None
    load = re.compile(r"(s_load_dword(?:x\d+)? \S+ s\[\d+:\d+\], )(0x[0-9a-f]+)$")
    add = re.compile(r"(s_add_u32 s(\d+), s(\d+), )(0x[0-9a-f]+)$")
    bases = {m.group(1) for ln in la for m in [re.match(r"s_load_dword(?:x\d+)? \S+ s\[(\d+):\d+\]", ln)] if m}
    loads, adds = set(), set()
    for x, y in zip(la, lb):
        if x == y:
            continue
        mx, my = load.match(x), load.match(y)
        if mx and my and mx.group(1) == my.group(1):
            loads.add((int(mx.group(2), 16), int(my.group(2), 16)))
            continue
        mx, my = add.match(x), add.match(y)
        if mx and my and mx.group(1) == my.group(1):
            adds.add((int(mx.group(4), 16), int(my.group(4), 16), mx.group(2) in bases or mx.group(3) in bases))
            continue
        return None
    deltas = {n - o for o, n in loads}
    if any(not base and (o, n) not in loads and (n - o) not in deltas for o, n, base in adds):
        return None
    return sorted(loads | {(o, n) for o, n, _ in adds})


def diff(a: str, b: str) -> int:
    """Symbols whose instructions differ.  Layout-only differences (padding, PC-relative offsets) are not
    differences; differences in kernel-argument offsets alone are listed apart with the offsets that moved;
    symbols present in one build only are listed and counted."""
    fa, fb = set(os.listdir(a)), set(os.listdir(b))
    bad = karg = 0
    moved = {}
    for f in sorted(fa | fb):
        if f not in fa or f not in fb:
            print(f"only in {'B' if f not in fa else 'A'}: {f}")
            continue
        la, lb = _normalise(open(os.path.join(a, f)).read()), _normalise(open(os.path.join(b, f)).read())
        if la == lb:
            continue
        pairs = _kernarg_only(la, lb)
        if pairs is not None:
            txt = ", ".join(f"{o:#x}->{n:#x}" for o, n in pairs)
            print(f"kernel-argument offsets only ({txt}): {f}")
            moved[txt] = moved.get(txt, 0) + 1
            karg += 1
            continue
        print(f"differs: {f}")
        bad += 1
    for txt, k in sorted(moved.items()):
        print(f"  offsets {txt}: {k} symbols")
    print(f"{len(fa & fb)} common symbols, {len(fa - fb)} only in A, {len(fb - fa)} only in B, {karg} with "
          f"kernel-argument offsets moved, {bad} with other differences")
    return bad + len(fa - fb)


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    if sys.argv[1] == "--regs":
        regs(sys.argv[2] if len(sys.argv) > 2 else "")
        sys.exit(0)
    print(f"{dump(sys.argv[1])} symbols")
