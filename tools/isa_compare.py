#!/usr/bin/env python3
"""isa_compare.py PARENT.so NEW.so -- compare the gfx950 code objects of two builds of csrc/liboffsim_hip.so, function by function.

The method of profiles/mlp_one_definition/isa_compare.txt: tools/extract_co.sh, llvm-objdump -d --no-show-raw-insn, then per function
a line-by-line comparison.  Normalised: addresses, the <symbol+offset> comments of branch targets, and the literal of the s_add_u32 /
s_addc_u32 pair after an s_getpc_b64 (the pc-relative distance to a global, which moves with the size of the code around it).  Nothing
else: register numbers and kernel-argument offsets count as differences.  Prints the counts, the identical instances by kernel, and for
every differing or one-sided instance the figures of the code object's notes, in the format of the reports under profiles/.  Needs no
GPU.  Exit status 0 whatever the outcome: the report is the result.  --defaulted-false: an instance of the new build whose template
argument list ends in `, false` is compared with the parent's instance without it (a kernel that gained a defaulted trailing parameter).
"""
import collections
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
HERE = os.path.dirname(os.path.abspath(__file__))
FIGURES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def functions(co):
    """{mangled symbol: [normalised instruction lines]} of the code object's .text"""
    out, name, after_getpc = collections.OrderedDict(), None, 0
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name, after_getpc = m.group(1), 0
            out[name] = []
            continue
        text = line.split("//")[0].strip()  # (drops the address and the <symbol+offset> of a branch target)
        if name is None or not text:
            continue
        if text.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc and re.match(r"s_addc?_u32 ", text):
            text = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", text)
            after_getpc -= 1
        out[name].append(text)
    return out


def notes(co):
    """{mangled symbol: {figure: int}} from the amdhsa.kernels metadata"""
    out, cur = {}, None
    for line in run(f"{LLVM}/llvm-readelf", "--notes", co).splitlines():
        if re.match(r"^\s{2}- \.", line):  # a new entry of amdhsa.kernels (its arguments are indented deeper)
            cur = {}
        m = re.match(r"^\s{2}(?:- |\s{2})\.(\w+):\s+(.*)$", line)
        if m and cur is not None:
            if m.group(1) == "name":
                out[m.group(2).strip("'\"")] = cur
            elif m.group(1) in FIGURES:
                cur[m.group(1)] = int(m.group(2))
    return out


def demangle(names):
    names = list(names)
    if not names:
        return {}
    tool = next((t for t in (f"{LLVM}/llvm-cxxfilt", shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if tool is None:  # (the report then shows the mangled names)
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, res))


def kernel_of(pretty):
    """'void k_eval_mc<float, ...>(...)' -> 'k_eval_mc'"""
    head = re.sub(r"^void ", "", pretty)
    return re.split(r"[<(]", head, maxsplit=1)[0]


def figures(n):
    if not n:
        return "(no note: a device function)"
    v = n.get("vgpr_count", 0)
    waves = min(8, 512 // max(8, (v + 7) // 8 * 8))  # gfx950: 512 VGPRs per SIMD lane, granule 8, at most 8 waves per SIMD
    return (f"vgpr={v} sgpr={n.get('sgpr_count', 0)} scratch={n.get('private_segment_fixed_size', 0)} lds_static={n.get('group_segment_fixed_size', 0)} "
            f"vgpr_spill={n.get('vgpr_spill_count', 0)} sgpr_spill={n.get('sgpr_spill_count', 0)} waves={waves}")


def by_kernel(names, pretty):
    c = collections.Counter(kernel_of(pretty[n]) for n in names)
    return "".join(f"  {k}: {c[k]}\n" for k in sorted(c)) or "  none\n"


def worse(p, b):
    """a figure of the branch worse than the parent's: more vgpr, scratch or vgpr_spill, or fewer waves per SIMD"""
    if not p or not b:
        return False
    w = lambda n: min(8, 512 // max(8, (n.get("vgpr_count", 0) + 7) // 8 * 8))  # noqa: E731
    return any(b.get(k, 0) > p.get(k, 0) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count")) or w(b) < w(p)


def main(parent_so, new_so, defaulted=False):
    renamed = []
    with tempfile.TemporaryDirectory() as tmp:
        cos = []
        for tag, so in (("parent", parent_so), ("branch", new_so)):
            co = os.path.join(tmp, tag + ".co")
            subprocess.run(["bash", os.path.join(HERE, "extract_co.sh"), so, co], check=True)
            cos.append(co)
        fp, fb = functions(cos[0]), functions(cos[1])
        np_, nb = notes(cos[0]), notes(cos[1])
    pretty = demangle(set(fp) | set(fb))
    if defaulted:  # a kernel that gained a defaulted trailing template parameter: its instance `..., false>(` is the parent's `...>(`
        by_pretty = {pretty[n]: n for n in fp if n not in fb}
        for n in [n for n in fb if n not in fp]:
            old = by_pretty.get(pretty[n].replace(", false>(", ">(", 1))
            if old is not None and ", false>(" in pretty[n]:
                fb = collections.OrderedDict((old if k == n else k, v) for k, v in fb.items())
                if n in nb:
                    nb[old] = nb.pop(n)
                renamed.append(pretty[n])
    both = [n for n in fp if n in fb]
    same = [n for n in both if fp[n] == fb[n]]
    diff = [n for n in both if fp[n] != fb[n]]
    only_p, only_b = [n for n in fp if n not in fb], [n for n in fb if n not in fp]
    w = sys.stdout.write
    w(f"functions in .text: parent {len(fp)}, branch {len(fb)}; identical line for line {len(same)}, different {len(diff)}, "
      f"in the parent only {len(only_p)}, in the branch only {len(only_b)}\n\n")
    if renamed:
        c = collections.Counter(kernel_of(p) for p in renamed)
        w("matched to the parent's instance by dropping a trailing defaulted `, false` template argument (instances): "
          + ", ".join(f"{k} {c[k]}" for k in sorted(c)) + "\n\n")
    w("identical line for line, by kernel (instances):\n" + by_kernel(same, pretty))
    w("\ndifferent (figures from the code object's notes; waves = waves per SIMD the VGPR count allows):\n")
    n_worse = 0
    for n in sorted(diff, key=lambda n: pretty[n]):
        sm = difflib.SequenceMatcher(None, fp[n], fb[n], autojunk=False)
        changed = sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in sm.get_opcodes() if op != "equal")
        w(f"  {pretty[n]}\n    instructions parent {len(fp[n])} branch {len(fb[n])}, lines that differ {changed}\n")
        w(f"    parent: {figures(np_.get(n))}\n    branch: {figures(nb.get(n))}\n")
        n_worse += worse(np_.get(n), nb.get(n))
    if not diff:
        w("  none\n")
    w(f"\ndifferent, by kernel (instances):\n" + by_kernel(diff, pretty))
    w(f"\ninstances with a figure worse than the parent's: {n_worse}\n")
    for tag, names, nt in (("parent", only_p, np_), ("branch", only_b, nb)):
        w(f"\nin the {tag} only, by kernel (instances):\n" + by_kernel(names, pretty))
        for n in sorted(names, key=lambda n: pretty[n]):
            w(f"  {pretty[n]}\n    {figures(nt.get(n))}\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--defaulted-false"]
    if len(args) != 2:
        sys.exit(__doc__)
    main(args[0], args[1], defaulted=len(args) != len(sys.argv) - 1)
