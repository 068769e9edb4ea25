#!/usr/bin/env python3
"""Instruction accounting of the gradient-kernel family's gfx950 machine code (CPU only, no GPU run).

    python scripts/isa_account.py <tag>                      -> profiles/isa_account_<tag>.txt
    python scripts/isa_account.py <tag> --compare OTHER_CSRC -> profiles/isa_compare_<tag>.txt   (two trees, kernel by kernel)
    python scripts/isa_account.py <tag> --preload OTHER_CSRC -> profiles/<tag>.txt   (kernel-argument preload length, registers, spills,
                                                                 scratch and segment s0 of the hot loop's kernels in two trees)

Compiles csrc/learner.hip device-only for gfx950 with _build.FLAGS (minus -shared / -ldl) plus -gline-tables-only, disassembles
it with source lines (llvm-objdump -d -l) and writes, for the gradient, reduce and acting kernels listed in KERNELS:

  * the instruction count per class (moves, nops, waits, LDS, global, MFMA, other VALU, scalar ALU, scalar memory, branches,
    lane reads and writes),
  * the count per segment between workgroup barriers,
  * the count per source line (top 40; the innermost inlined frame, as the line table gives it),
  * the runs of six or more consecutive register moves, with their source lines,
  * the descriptor figures of the metadata note: VGPR, AGPR, SGPR, spills, scratch.

It lists what is in the listing, class by mnemonic prefix; it looks for no particular instruction.  -gline-tables-only changes
no instruction: the tool checks that by comparing the per-kernel instruction counts with a build without it (--check-lines).

--compare builds learner.hip, uavenv.hip, sac.hip and replay.hip of two trees without line tables and sets every kernel's listing
and descriptor figures side by side: identical or not, instruction counts, registers, spills, scratch, waves per SIMD; the kernels of
MUST_MATCH and of MUST_MATCH_FILES have to be identical (exit status 1 otherwise).  --diff-lines N prints the listing diff.
"""
from __future__ import annotations

import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dqn_based_uav_3d_path_planer_amd import _build  # noqa: E402

KERNELS = ["k_dqn_grad_packed8<true>", "k_dqn_grad_packed8<false>", "k_dqn_grad_slots<true>", "k_dqn_grad_slots<false>",
           "k_dqn_grad_slots_w<true>", "k_dqn_grad_slots_w<false>",
           "k_dqn_reduce_adam", "k_dqn_reduce_adam_slots",
           "k_dqn_act<float, 4>", "k_dqn_act<float, 14>", "k_dqn_act<__half, 4>", "k_dqn_act<__half, 14>",
           "k_dqn_act_packed<4>", "k_dqn_act_packed<14>", "k_dqn_act_slots<4>", "k_dqn_act_slots<14>",
           "k_dqn_act_h<1, 4>", "k_dqn_act_h<2, 4>"]
# --compare: the kernels whose instruction stream has to be the other tree's, instruction for instruction (the single-learner loops
# and the benchmark are timed on them), next to every kernel of the files in MUST_MATCH_FILES
MUST_MATCH = ["k_dqn_grad_packed8<true>", "k_dqn_grad_packed8<false>", "k_dqn_reduce_adam"]
MUST_MATCH_FILES = ["uavenv", "sac", "replay"]
COMPARE_FILES = ["learner"] + MUST_MATCH_FILES
CLASSES = ["move", "nop", "wait", "barrier", "lds", "global", "mfma", "lane", "valu", "smem", "branch", "salu"]
CLASS_TEXT = {"move": "register moves (v_mov_*)", "nop": "nops (s_nop)", "wait": "waits (s_waitcnt*)", "barrier": "workgroup barriers",
              "lds": "LDS (ds_*)", "global": "global / flat / buffer / scratch", "mfma": "MFMA (v_mfma_*)",
              "lane": "lane reads and writes (v_readlane / v_writelane / v_readfirstlane)", "valu": "other VALU (v_*)",
              "smem": "scalar memory loads (s_load_* / s_buffer_load_*)", "branch": "branches (s_branch / s_cbranch_* / s_setpc / s_endpgm)",
              "salu": "scalar ALU and the rest (s_*)"}


def classify(m: str) -> str:
    if m.startswith("v_mov_"):
        return "move"
    if m == "s_nop":
        return "nop"
    if m.startswith("s_waitcnt"):
        return "wait"
    if m == "s_barrier":
        return "barrier"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global"
    if m.startswith(("v_mfma", "v_smfma")):
        return "mfma"
    if m.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if m.startswith("v_"):
        return "valu"
    if m.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if m.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_endpgm", "s_call")):
        return "branch"
    return "salu"


def tool(name: str) -> str:
    hipcc = _build._hipcc()
    for d in (os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin"),
              os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return name


def compile_device(src: str, out: str, lines: bool, unit_flags: bool = True, asm: bool = False) -> None:
    """unit_flags: with _build.unit_flags of the file (kernel-argument preload); False builds a tree from before them as it was built"""
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-ldl")]
    if unit_flags:
        flags += _build.unit_flags(os.path.basename(src))
    cmd = [_build._hipcc()] + flags + (["-gline-tables-only"] if lines else []) + \
          ["--cuda-device-only", "--no-gpu-bundle-output", "-S" if asm else "-c", src, "-o", out]
    subprocess.run(cmd, check=True)


def short_name(sym: str) -> str:
    """'void (anonymous namespace)::k_x<true>((anonymous namespace)::Grad2Args)' -> 'k_x<true>'"""
    s = sym.replace("(anonymous namespace)::", "")
    s = re.sub(r"^void ", "", s)
    depth = 0
    for i, ch in enumerate(s):                         # cut the argument list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i]
    return s


def disassemble(obj: str, lines: bool):
    """{short kernel name: [(mnemonic, operands, 'file:line' or '')]} for every function symbol of the object"""
    cmd = [tool("llvm-objdump"), "-d", "--no-show-raw-insn", "-C"] + (["-l"] if lines else []) + [obj]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    out, cur, loc = {}, None, ""
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", ln)
        if m:
            cur = out.setdefault(short_name(m.group(1)), [])
            loc = ""
            continue
        if cur is None or not ln.strip():
            continue
        s = ln.strip()
        if s.startswith(";"):
            m = re.match(r"^; (\S+):(\d+)$", s)
            if m:
                loc = "%s:%s" % (os.path.basename(m.group(1)), m.group(2))
            continue
        if s.startswith("...") or s.endswith(":") and " " not in s:
            continue
        body = s.split("//")[0].strip()
        if not body:
            continue
        parts = body.split(None, 1)
        cur.append((parts[0], parts[1] if len(parts) > 1 else "", loc))
    return out


def demangle_map(obj: str) -> dict:
    """{mangled: demangled} of the object's symbols: the symbol table printed twice, plain and with -C, line for line"""
    raw = subprocess.run([tool("llvm-objdump"), "-t", obj], check=True, capture_output=True, text=True).stdout.splitlines()
    dem = subprocess.run([tool("llvm-objdump"), "-t", "-C", obj], check=True, capture_output=True, text=True).stdout.splitlines()
    out = {}
    for a, b in zip(raw, dem):
        m = re.match(r"^[0-9a-f]{16} .{7} \S+\t[0-9a-f]+ (?:\.\w+ )?(.*)$", a)
        if not m:
            continue
        out[m.group(1)] = b[len(a) - len(m.group(1)):]
    return out


def descriptors(obj: str):
    """{short kernel name: {figure: value}} from the AMDGPU metadata note"""
    text = subprocess.run([tool("llvm-readelf"), "--notes", obj], check=True, capture_output=True, text=True).stdout
    keys = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".vgpr_spill_count": "vgpr_spills",
            ".sgpr_spill_count": "sgpr_spills", ".private_segment_fixed_size": "scratch", ".group_segment_fixed_size": "static_lds"}
    kernels, cur = [], None
    for ln in text.splitlines():
        m = re.match(r"^  - (\.\w+):\s*(.*)$", ln)                     # a kernel's map begins at a list item of the outer list
        if m:
            cur = {}
            kernels.append(cur)
        else:
            m = re.match(r"^    (\.\w+):\s*(.*)$", ln)
        if not m or cur is None:
            continue
        k, v = m.group(1), m.group(2).strip().strip("'")
        if k in keys:
            cur[keys[k]] = int(v)
        elif k == ".name":
            cur["name"] = v
    names = demangle_map(obj)
    return {short_name(names.get(d["name"], d["name"])): d for d in kernels if "name" in d}


def account(name: str, ins, desc) -> list:
    L = []
    L.append("=" * 100)
    L.append("%s: %d instructions" % (name, len(ins)))
    if desc:
        L.append("  descriptor: vgpr %d  agpr %d  sgpr %d  spills vgpr %d / sgpr %d  scratch %d B  static lds %d B" % (
            desc.get("vgpr", -1), desc.get("agpr", -1), desc.get("sgpr", -1), desc.get("vgpr_spills", -1), desc.get("sgpr_spills", -1),
            desc.get("scratch", -1), desc.get("static_lds", -1)))
    cls = [classify(m) for m, _, _ in ins]
    # ---- segments between workgroup barriers
    bars = [i for i, c in enumerate(cls) if c == "barrier"]
    edges = [0] + bars + [len(ins)]
    # blocks that the compiler lays out behind the kernel's end (out-of-line arms of earlier branches) are no part of the last
    # segment's straight-line code: they get a column of their own
    ends = [i for i, (m, _, _) in enumerate(ins) if m == "s_endpgm" and i > (bars[-1] if bars else -1)]
    ool = bool(ends) and ends[0] + 1 < len(ins)
    if ool:
        edges = edges[:-1] + [ends[0] + 1, len(ins)]
    seg_name = ["s%d" % k for k in range(len(edges) - 1)]
    if ool:
        seg_name[-1] = "ool"
    L.append("")
    L.append("  per class, whole kernel and per segment between workgroup barriers (barriers at instruction %s)" % (
        ", ".join(str(b) for b in bars) or "-"))
    head = "    %-9s %7s" % ("class", "all") + "".join(" %6s" % n for n in seg_name)
    L.append(head)
    for c in CLASSES:
        row = "    %-9s %7d" % (c, cls.count(c))
        for k in range(len(edges) - 1):
            row += " %6d" % cls[edges[k]:edges[k + 1]].count(c)
        L.append(row)
    row = "    %-9s %7d" % ("total", len(ins))
    for k in range(len(edges) - 1):
        row += " %6d" % (edges[k + 1] - edges[k])
    L.append(row)
    L.append("    (segment = instructions [start, end): " + "  ".join(
        "%s [%d, %d)" % (seg_name[k], edges[k], edges[k + 1]) for k in range(len(edges) - 1)) +
        ("; ool = blocks laid out behind the kernel's s_endpgm" if ool else "") + ")")
    # ---- per source line
    per = collections.Counter(loc or "(no line)" for _, _, loc in ins)
    mv = collections.Counter(loc or "(no line)" for (_, _, loc), c in zip(ins, cls) if c == "move")
    L.append("")
    L.append("  per source line, top 40 (instructions, of which moves)")
    for loc, n in per.most_common(40):
        L.append("    %6d %5d  %s" % (n, mv.get(loc, 0), loc))
    # ---- move runs
    L.append("")
    runs, i = [], 0
    while i < len(ins):
        if cls[i] == "move":
            j = i
            while j < len(ins) and cls[j] == "move":
                j += 1
            if j - i >= 6:
                runs.append((i, j))
            i = j
        else:
            i += 1
    L.append("  runs of six or more consecutive moves: %d runs, %d moves" % (len(runs), sum(b - a for a, b in runs)))
    for a, b in runs:
        seg = max(k for k in range(len(edges) - 1) if edges[k] <= a)
        locs = collections.Counter(ins[k][2] or "(no line)" for k in range(a, b))
        L.append("    at %5d (%s) length %2d: %s" % (a, seg_name[seg], b - a, ", ".join("%s x%d" % kv for kv in locs.most_common(4))))
    L.append("")
    return L


def waves_per_simd(desc) -> int:
    """occupancy step of a gfx950 kernel from its unified register count (the note's vgpr figure is VGPRs + AGPRs): 512 per lane
    and SIMD, allocated in eights, 8 waves at most"""
    regs = (desc.get("vgpr", 0) + 7) // 8 * 8
    return min(8, 512 // max(regs, 8))


def compare(other_csrc: str, this_csrc: str, diff_lines: int, files) -> tuple:
    """(report lines, ok): every kernel of COMPARE_FILES in `other_csrc` against the same kernel in `this_csrc`, built without line
    tables: (mnemonic, operands) sequences (addresses and branch-target annotations are no part of them; a branch's operand is its
    relative distance) and the descriptor figures"""
    import difflib
    FIG = ["vgpr", "agpr", "sgpr", "vgpr_spills", "sgpr_spills", "scratch", "static_lds"]
    L, ok = [], True
    with tempfile.TemporaryDirectory() as td:
        from concurrent.futures import ThreadPoolExecutor

        def build(job):
            side, csrc, f = job
            obj = os.path.join(td, "%s_%s.o" % (f, side))
            compile_device(os.path.join(csrc, f + ".hip"), obj, False, tree_has_unit_flags(csrc))
            return (side, f), (disassemble(obj, False), descriptors(obj))
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            built = dict(ex.map(build, [(side, csrc, f) for side, csrc in (("a", other_csrc), ("b", this_csrc)) for f in files]))
    for f in files:
        (da, ka), (db, kb) = built["a", f], built["b", f]
        L.append("=" * 100)
        L.append("%s.hip: %d kernels in the other tree, %d in this tree" % (f, len(ka), len(kb)))
        L.append("  %-58s %7s %7s  %-9s %s" % ("kernel", "other", "this", "stream", "descriptor (vgpr agpr sgpr spills v/s scratch lds; waves/SIMD)"))
        for k in sorted(set(ka) | set(kb)):
            if k not in ka or k not in kb:
                L.append("  %-58s only in %s tree" % (k, "the other" if k in ka else "this"))
                if k in ka and (f in MUST_MATCH_FILES or k in MUST_MATCH):        # a must-match kernel is gone; a new kernel moves none
                    ok = False
                continue
            sa, sb = [(m, o) for m, o, _ in da[k]], [(m, o) for m, o, _ in db[k]]
            fa, fb = [ka[k].get(x, -1) for x in FIG], [kb[k].get(x, -1) for x in FIG]
            same = sa == sb and fa == fb
            must = f in MUST_MATCH_FILES or k in MUST_MATCH
            fig = lambda v, d: "%d %d %d %d/%d %d %d; %d" % (v[0], v[1], v[2], v[3], v[4], v[5], v[6], waves_per_simd(d))
            L.append("  %-58s %7d %7d  %-9s %s%s" % (k, len(sa), len(sb), "identical" if sa == sb else "DIFFERENT",
                                                   fig(fa, ka[k]) if fa == fb else "%s -> %s" % (fig(fa, ka[k]), fig(fb, kb[k])),
                                                   "   <-- MUST MATCH" if must and not same else ""))
            if must and not same:
                ok = False
            if sa != sb and diff_lines:
                ta, tb = ["%s %s" % x for x in sa], ["%s %s" % x for x in sb]
                d = [x for x in difflib.unified_diff(ta, tb, "other", "this", n=1, lineterm="")][2:]
                L.append("      %d lines removed, %d added" % (sum(x.startswith("-") for x in d), sum(x.startswith("+") for x in d)))
                L += ["      " + x for x in d[:diff_lines]]
                if len(d) > diff_lines:
                    L.append("      ... (%d more diff lines)" % (len(d) - diff_lines))
    L.append("")
    L.append("gate (identical stream and descriptor for %s and every kernel of %s): %s" % (
        ", ".join(MUST_MATCH), ", ".join(x + ".hip" for x in MUST_MATCH_FILES), "HOLDS" if ok else "BROKEN"))
    return L, ok


PRELOAD_KERNELS = [("uavenv", "k_step_coop<unsigned int, false, 2, true, true, true>"), ("learner", "k_dqn_grad_packed8<true>"),
                   ("learner", "k_dqn_reduce_adam"), ("learner", "k_dqn_reduce_adam_slots")]


def tree_has_unit_flags(csrc: str) -> bool:
    """does the tree that holds `csrc` build with per-unit flags (its _build.py, next to csrc, defines unit_flags)?"""
    b = os.path.join(csrc, "..", "_build.py")
    return os.path.exists(b) and "def unit_flags" in open(b).read()


def preload_lengths(asm: str, names: dict) -> dict:
    """{short kernel name: .amdhsa_user_sgpr_kernarg_preload_length} of an assembly listing (the kernel descriptor's field);
    names: demangle_map of the same file's object"""
    text = open(asm).read()
    found = re.findall(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s+\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", text)
    return {short_name(names.get(sym, sym)): int(n) for sym, n in found}


def preload_report(other_csrc: str, this_csrc: str) -> list:
    """The three hot-loop kernels in a tree from before kernel-argument preload (built without unit flags) and in this tree: the
    descriptor's preload length, registers, spills, scratch, and the instruction count of segment s0 (up to the first barrier)"""
    L = ["  %-58s %-6s %8s %5s %5s %12s %8s %7s %6s" % ("kernel", "tree", "preload", "vgpr", "sgpr", "spills v/s", "scratch", "total", "s0")]
    with tempfile.TemporaryDirectory() as td:
        for f in sorted(set(f for f, _ in PRELOAD_KERNELS)):
            for side, csrc, uf in (("other", other_csrc, tree_has_unit_flags(other_csrc)), ("this", this_csrc, True)):
                obj, asm = os.path.join(td, "%s_%s.o" % (f, side)), os.path.join(td, "%s_%s.s" % (f, side))
                compile_device(os.path.join(csrc, f + ".hip"), obj, False, uf)
                compile_device(os.path.join(csrc, f + ".hip"), asm, False, uf, asm=True)
                dis, desc, pre = disassemble(obj, False), descriptors(obj), preload_lengths(asm, demangle_map(obj))
                for ff, k in PRELOAD_KERNELS:
                    if ff != f:
                        continue
                    ins, d = dis[k], desc[k]
                    bars = [i for i, (m, _, _) in enumerate(ins) if classify(m) == "barrier"]
                    L.append("  %-58s %-6s %8d %5d %5d %12s %8d %7d %6d" % (
                        k, side, pre[k], d["vgpr"], d["sgpr"], "%d / %d" % (d["vgpr_spills"], d["sgpr_spills"]), d["scratch"], len(ins),
                        bars[0] if bars else len(ins)))
    return L


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tag")
    ap.add_argument("--compare", metavar="CSRC", default=None,
                    help="compare mode: the csrc directory of another tree (e.g. an export of the parent commit); writes "
                         "profiles/isa_compare_<tag>.txt and exits 1 if a must-match kernel moved")
    ap.add_argument("--files", nargs="+", choices=COMPARE_FILES, default=None, help="compare mode: only these files (default: all four)")
    ap.add_argument("--diff-lines", type=int, default=0, help="compare mode: print up to this many diff lines per changed kernel")
    ap.add_argument("--csrc", default=_build.CSRC, help="directory holding learner.hip (default: this tree's csrc)")
    ap.add_argument("--out", default=None, help="output file (default profiles/isa_account_<tag>.txt)")
    ap.add_argument("--check-lines", action="store_true", help="also build without -gline-tables-only and compare the counts")
    ap.add_argument("--preload", metavar="CSRC", default=None,
                    help="kernel-argument preload report of the three hot-loop kernels against the csrc directory of a tree from before "
                         "it; writes profiles/<tag>.txt")
    args = ap.parse_args()
    if args.preload:
        out = args.out or os.path.join(ROOT, "profiles", "%s.txt" % args.tag)
        with open(out, "w") as f:
            f.write("\n".join(preload_report(args.preload, args.csrc)) + "\n")
        print(out)
        return 0
    if args.compare:
        L, ok = compare(args.compare, args.csrc, args.diff_lines, args.files or COMPARE_FILES)
        flags = " ".join(f for f in _build.FLAGS if f not in ("-shared", "-ldl"))
        head = ["Listing comparison, tag '%s' (scripts/isa_account.py --compare; CPU only): 'other' = the tree given, 'this' = this tree." % args.tag,
                "  hipcc %s --cuda-device-only --no-gpu-bundle-output -c <file>.hip ; llvm-objdump -d --no-show-raw-insn -C ; llvm-readelf --notes" % flags,
                "A stream is the sequence of (mnemonic, operands); instruction counts are given per kernel.", ""]
        out = args.out or os.path.join(ROOT, "profiles", "isa_compare_%s.txt" % args.tag)
        with open(out, "w") as f:
            f.write("\n".join(head + L) + "\n")
        print(out)
        return 0 if ok else 1
    src = os.path.join(args.csrc, "learner.hip")
    out = args.out or os.path.join(ROOT, "profiles", "isa_account_%s.txt" % args.tag)
    with tempfile.TemporaryDirectory() as td:
        obj = os.path.join(td, "learner_lines.o")
        compile_device(src, obj, True)
        dis = disassemble(obj, True)
        desc = descriptors(obj)
        plain = None
        if args.check_lines:
            obj2 = os.path.join(td, "learner_plain.o")
            compile_device(src, obj2, False)
            plain = disassemble(obj2, False)
    flags = " ".join(f for f in _build.FLAGS if f not in ("-shared", "-ldl"))
    L = ["Instruction accounting of csrc/learner.hip's gradient-kernel family, tag '%s' (scripts/isa_account.py; CPU only)." % args.tag,
         "  hipcc %s -gline-tables-only --cuda-device-only --no-gpu-bundle-output -c learner.hip" % flags,
         "  llvm-objdump -d -l --no-show-raw-insn -C ; llvm-readelf --notes",
         "Counts are instructions proper (labels, source-line comments and the zero padding behind a kernel are not counted).",
         "Source lines are the innermost inlined frame of the line table.", ""]
    missing = [k for k in KERNELS if k not in dis]
    if missing:
        print("kernels not found in the listing: %s\nhave: %s" % (missing, sorted(dis)), file=sys.stderr)
        return 1
    for k in KERNELS:
        L += account(k, dis[k], desc.get(k))
        if plain is not None:
            same = [a[0] for a in plain[k]] == [a[0] for a in dis[k]]
            L.append("  without -gline-tables-only: %d instructions, mnemonic stream %s" % (len(plain[k]), "identical" if same else "DIFFERENT"))
            L.append("")
    with open(out, "w") as f:
        f.write("\n".join(L))
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
