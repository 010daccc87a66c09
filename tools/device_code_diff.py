"""Compares the gfx950 device code of this tree with that of another checkout, unit by unit and kernel by kernel.

    python tools/device_code_diff.py OTHER_TREE [-j JOBS] [-o REPORT] [UNIT.hip ...]

OTHER_TREE is a checkout of the commit to compare against (e.g. `git worktree add ../parent HEAD~1`, made by whoever runs the
tool).  Every stereo-depth_amd/csrc/*.hip of both trees is compiled to assembly with the flags of this tree's build.py
(per-file flags included) plus `--cuda-device-only -S`, from inside its own csrc directory so that no path differs.  The
`__hip_cuid_<hash>` symbol, `.file` / `.ident` lines and comment lines are masked.  Per unit, and per function symbol of a
unit that differs, the report says: identical or not, the count of differing lines, the diff, and what the `amdhsa.kernels`
metadata says about the kernel on either side (registers, spills, private and group segment).  The tool compares text and
nothing else.  Exit status: 0 when every unit is identical, 1 otherwise.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "stereo-depth_amd"
META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")


def load_build():
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_unit(build, tree: str, unit: str, out: str) -> None:
    csrc = os.path.join(tree, PKG, "csrc")
    cmd = ([build.hipcc()] + build.FLAGS + os.environ.get("SMX_EXTRA_FLAGS", "").split() + ["-I", os.path.join("..", "..", "include")] +
           build.PER_FILE_FLAGS.get(unit, []) + ["--cuda-device-only", "-S", "-o", out, unit])
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {unit} of {tree}:\n{r.stdout}{r.stderr}")


def masked(path: str) -> list[str]:
    lines = []
    for line in open(path):
        t = line.strip()
        if not t or t.startswith(";") or t.startswith("//") or t.startswith(".file") or t.startswith(".ident"):
            continue
        lines.append(re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", line.rstrip()))
    return lines


def functions(lines: list[str]) -> dict[str, list[str]]:
    """The unit's text by function symbol (from its `.type sym,@function` to the next one); what precedes the first
    function and the metadata note at the end are the segments `<head>` and `<metadata>`."""
    segs: dict[str, list[str]] = {"<head>": []}
    cur = "<head>"
    for line in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            # the .globl / .p2align / .protected lines in front of .type belong to the function as well
            moved = []
            prev = segs[next(reversed(segs))]
            while prev and re.match(r"\s*\.(globl|p2align|protected|weak|hidden|section|text)\b", prev[-1]):
                moved.insert(0, prev.pop())
            segs[cur] = moved
        elif line.strip() == ".amdgpu_metadata":
            cur = "<metadata>"
            segs[cur] = []
        segs[cur].append(line)
    return segs


def kernel_metadata(lines: list[str]) -> dict[str, dict[str, str]]:
    """{kernel symbol: {key: value}} from the amdhsa.kernels list of the metadata note."""
    out: dict[str, dict[str, str]] = {}
    entry: dict[str, str] | None = None
    inside = False
    for line in lines:
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if re.match(r"\S", line):
            break
        m = re.match(r"  (- | {2})\.(\w+):\s*(.*)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            entry = {}
        if entry is not None:
            entry[m.group(2)] = m.group(3).strip().strip("'")
            if m.group(2) == "name":
                out[entry["name"]] = entry
    return out


def instruction_lines(seg: list[str]) -> int:
    return sum(1 for s in seg if not s.lstrip().startswith(".") and not s.rstrip().endswith(":"))


def text_diff(a: list[str], b: list[str], tmp: str) -> list[str]:
    pa, pb = os.path.join(tmp, "a.txt"), os.path.join(tmp, "b.txt")
    for p, seg in ((pa, a), (pb, b)):
        with open(p, "w") as f:
            f.write("\n".join(seg) + "\n")
    r = subprocess.run(["diff", "-U2", "--label", "other", "--label", "this", pa, pb], capture_output=True, text=True)
    return r.stdout.splitlines()


def changed(diff: list[str]) -> int:
    return sum(1 for s in diff if (s.startswith("+") or s.startswith("-")) and not s.startswith(("+++", "---")))


def meta_line(meta: dict[str, str] | None) -> str:
    if meta is None:
        return "(no kernel descriptor)"
    return " ".join(f"{k}={meta.get(k, '?')}" for k in META_KEYS)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("other_tree")
    ap.add_argument("units", nargs="*", help="only these csrc/*.hip (default: all of both trees)")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("-o", "--output", help="write the report here as well")
    args = ap.parse_args()
    build = load_build()
    trees = {"other": os.path.abspath(args.other_tree), "this": ROOT}
    names = {k: {f for f in os.listdir(os.path.join(t, PKG, "csrc")) if f.endswith(".hip")} for k, t in trees.items()}
    units = sorted(args.units or (names["other"] | names["this"]))
    report: list[str] = []
    differing = 0
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for k, t in trees.items():
            os.makedirs(os.path.join(tmp, k))
            jobs += [(t, u, os.path.join(tmp, k, u[:-4] + ".s")) for u in units if u in names[k]]
        jobs.sort(key=lambda j: -os.path.getsize(os.path.join(j[0], PKG, "csrc", j[1])))
        with ThreadPoolExecutor(max_workers=max(1, min(args.jobs, 8))) as pool:
            list(pool.map(lambda j: compile_unit(build, *j), jobs))
        report.append(f"device code of {len(units)} units, other tree against this one (masked: __hip_cuid_*, .file, .ident, comments)")
        for u in units:
            if u not in names["other"] or u not in names["this"]:
                differing += 1
                report.append(f"{u}: ONLY IN {'this' if u in names['this'] else 'other'} tree")
                continue
            a, b = (masked(os.path.join(tmp, k, u[:-4] + ".s")) for k in ("other", "this"))
            fa, fb = functions(a), functions(b)
            ma, mb = kernel_metadata(a), kernel_metadata(b)
            if a == b:
                report.append(f"{u}: identical ({len(ma)} kernels, {len(a)} lines)")
                continue
            differing += 1
            report.append(f"{u}: DIFFERS ({len(ma)} / {len(mb)} kernels, {len(a)} / {len(b)} lines, {changed(text_diff(a, b, tmp))} differing lines)")
            for sym in list(fa) + [s for s in fb if s not in fa]:
                sa, sb = fa.get(sym), fb.get(sym)
                if sa == sb:
                    report.append(f"  {sym}: identical")
                    continue
                if sa is None or sb is None:
                    report.append(f"  {sym}: ONLY IN {'this' if sa is None else 'other'} tree")
                    continue
                d = text_diff(sa, sb, tmp)
                report.append(f"  {sym}: DIFFERS, {changed(d)} differing lines, instruction lines {instruction_lines(sa)} / {instruction_lines(sb)}")
                if sym in ma or sym in mb:
                    report.append(f"    other: {meta_line(ma.get(sym))}")
                    report.append(f"    this:  {meta_line(mb.get(sym))}")
                report += ["    " + s for s in d]
        report.append(f"{len(units) - differing} of {len(units)} units identical")
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
