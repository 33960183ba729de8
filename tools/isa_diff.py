"""Device code of two builds, function by function: for every object file of two directories that each hold the objects of a plain `make`, extracts the
gfx950 code object, disassembles it, cuts the text into functions and compares each function's instruction text with addresses, encodings, branch-target
labels and the padding between functions removed.  Whole texts are compared; no instruction is looked for.  No GPU needed.
    python tools/isa_diff.py PARENT_CSRC TREE_CSRC -> one line per function: object, same / differs / gone / new, instructions in the parent and in the
    tree, demangled name (no parameter list, no `(anonymous namespace)::`); kernels: VGPRs, SGPRs, LDS bytes, scratch bytes as parent -> tree; a function that differs: whether its floating-point opcodes are the parent's in order
    python tools/isa_diff.py PARENT_CSRC TREE_CSRC OBJECT FUNCTION -> the unified diff of that function's instruction text"""
import glob, os, re, shutil, subprocess, sys, tempfile
LLVM = "/opt/rocm/llvm/bin/"
META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def functions(obj, tmp):
    """{short name: (instruction lines, kernel metadata or None)} of one object file's gfx950 code object"""
    work = os.path.join(tmp, os.path.basename(obj))  # (the extraction writes next to its input)
    shutil.copy(obj, work)
    subprocess.check_output([LLVM + "llvm-objdump", "--offloading", work])
    co = glob.glob(work + ".*gfx950")
    if not co:
        return {}
    meta = {}
    for rec in subprocess.check_output([LLVM + "llvm-readelf", "--notes", co[0]], text=True).split("\n  - ")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
        if "vgpr_count" in f:
            meta[f["name"]] = tuple(int(f[k]) for k in META)
    out = {}
    plain, nice = (subprocess.check_output([LLVM + "llvm-objdump", "-d"] + c + [co[0]], text=True) for c in ([], ["-C"]))
    heads = zip(re.finditer(r"^[0-9a-f]+ <(.*)>:$", plain, re.M), re.finditer(r"^[0-9a-f]+ <(.*)>:$", nice, re.M))
    bodies = re.split(r"^[0-9a-f]+ <.*>:$", plain, flags=re.M)[1:]
    for (m, n), body in zip(heads, bodies):
        ins = [l.split("//")[0].strip() for l in body.splitlines()]
        ins = [l for l in ins if l and l != "..." and not l.startswith("Disassembly of")]
        while ins and ins[-1].split()[0] in ("s_nop", "s_code_end"):  # padding behind the last instruction
            ins.pop()
        short = re.sub(r"\(anonymous namespace\)::", "", n.group(1))
        short = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", short)
        out[short] = (ins, meta.get(m.group(1)))
    return out


def float_ops(ins):
    """the opcodes of the floating-point instructions of a function, in order: v_* on f32 / f64 (conversions included) and the rcp / sqrt / rsq forms"""
    ops = [l.split()[0] for l in ins]
    return [o for o in ops if o.startswith("v_") and re.search(r"f32|f64|rcp|sqrt|rsq", o)]


def main(parent, tree):
    count = {"same": 0, "differs": 0, "gone": 0, "new": 0}
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        names = sorted({os.path.basename(p) for d in (parent, tree) for p in glob.glob(os.path.join(d, "*.o"))})
        for o in names:
            a, b = (functions(os.path.join(d, o), t) if os.path.exists(os.path.join(d, o)) else {} for d, t in ((parent, ta), (tree, tb)))
            for f in sorted(set(a) | set(b)):
                (ia, ma), (ib, mb) = a.get(f, ([], None)), b.get(f, ([], None))
                what = "gone" if f not in b else "new" if f not in a else "same" if ia == ib else "differs"
                count[what] += 1
                res = ""
                if ma or mb:
                    res = "  " + " ".join(f"{k} {x if x == y else f'{x} -> {y}'}" for k, x, y in zip(("vgpr", "sgpr", "lds", "scratch"), ma or ("-",) * 4, mb or ("-",) * 4))
                if what == "differs":  # is the arithmetic the parent's?  The floating-point opcodes in order, operands aside
                    fa, fb = float_ops(ia), float_ops(ib)
                    res += f"  float opcodes {len(fa)} -> {len(fb)}, {'the same sequence' if fa == fb else 'ANOTHER sequence'}"
                print(f"{o:28s} {what:8s} {len(ia):6d} {len(ib):6d}  {f}{res}")
    print("\n" + ", ".join(f"{v} {k}" for k, v in count.items()))


def show(parent, tree, obj, func):
    import difflib
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = (functions(os.path.join(d, obj), t)[func][0] for d, t in ((parent, ta), (tree, tb)))
    print("\n".join(difflib.unified_diff(a, b, "parent", "tree", lineterm="", n=2)))


if __name__ == "__main__":
    show(*sys.argv[1:5]) if len(sys.argv) > 3 else main(*sys.argv[1:3])
