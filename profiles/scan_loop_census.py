"""Instruction census of the packed-filter loops of the sphere-list kernel (kind 16; render.hip scan_filtered32).

Compiles render.hip to gfx950 assembly with the flags csrc/Makefile uses for render_strict.o and render_fast.o, finds every loop
that runs the packed fp32 filter (v_pk_mul_f32 / v_pk_fma_f32 on scalar rows) and walks one trip of it along the QUIET path -- the
path of a trip in which no lane passes any sphere -- counting what the wave issues there and how far ahead of its wait every
scalar load is issued.  There are two such loops per scan: the GENERAL form (a v_pk_mul_f32 opens every s chain: 7 packed
instructions per pair of spheres) and the RUN form of a segment whose rows share a centre coordinate (no multiply on a scalar
row: 5 per pair).  The loop over the segments that holds both is not a trip of either and is left out.

The quiet path is followed by these rules: a ballot compared with zero is zero; the drain test (v_cmp_lt_u32 on the queue count)
is false; exec is not empty; a conditional branch to the loop's header is taken; any other conditional branch out of the loop is
not.  A branch the rules do not decide is reported and assumed not taken.

    python profiles/scan_loop_census.py [--src path/to/render.hip] [--label text] [--keep DIR]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# csrc/Makefile DEVFLAGS, and what it adds for the two plain objects
DEVFLAGS = ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950", "-Wall", "-Wno-unused-parameter",
            "-Wno-unused-value", "-Wno-unneeded-internal-declaration"]
BUILDS = {"strict": ["-DRT_STRICT=1", "-ffp-contract=off"], "fast": ["-DRT_STRICT=0", "-ffp-contract=fast"]}

FILTER = ("v_pk_mul_f32", "v_pk_fma_f32", "v_cmp_lt_f32")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
HEADER_OF = re.compile(r"in Loop: Header=(BB\d+_\d+)")


def assemble(src, build, keep):
    out = os.path.join(keep, f"render_{build}.s")
    cmd = [HIPCC] + DEVFLAGS + BUILDS[build] + ["--cuda-device-only", "-S", os.path.basename(src), "-o", out]
    subprocess.run(cmd, cwd=os.path.dirname(src), check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read().splitlines()


def functions(lines):
    """(name, first line, last line) of every function of the assembly file."""
    out, name, start = [], None, 0
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, start = m.group(1), i
        elif ln.startswith(".Lfunc_end") and name:
            out.append((name, start, i))
            name = None
    return out


def op_of(ln):
    s = ln.strip()
    if not s or s[0] in ";." or s.startswith(";;#") or LABEL.match(s):
        return None
    return s.split()[0]


SQUARE = re.compile(r"v_pk_fma_f32 v\[\d+:\d+\], (v\[\d+:\d+\]), \1,")  # q = fma(s, s, ...): one per pair of spheres


def quiet_trip(lines, lo, hi, header, headers=()):
    """Walk one trip from the header's label along the quiet path: list of (line index, text, taken?) and notes.  A path that
    enters another loop of `headers` is the trip of an outer loop: returns (None, notes)."""
    labels = {}
    in_loop = set()
    for i in range(lo, hi):
        m = LABEL.match(lines[i])
        if m:
            labels[m.group(1)] = i
            h = HEADER_OF.search(lines[i])
            if h and "." + "L" + h.group(1) == header:
                in_loop.add(m.group(1))
    # a fall-through block (; %bb.N:) carries its loop in a comment too, but has no label: only labelled targets matter here
    path, notes = [], []
    i = labels[header] + 1
    scc = vcc = None  # value on the quiet path when the rules know it
    for _ in range(4000):
        ln = lines[i]
        m = LABEL.match(ln)
        if m and m.group(1) == header:
            break
        if m and m.group(1) in headers:
            return None, [f"enters loop {m.group(1)}"]
        op = op_of(ln)
        if op is None:
            i += 1
            continue
        s = ln.strip()
        taken = None
        if op.startswith("s_cmp_"):
            args = [a.strip() for a in s[len(op):].split(",")]
            scc = None
            if op in ("s_cmp_eq_u64", "s_cmp_lg_u64") and args[-1] == "0":
                scc = 1 if op == "s_cmp_eq_u64" else 0
        elif op.startswith("v_cmp") and s[len(op):].split(",")[0].strip() == "vcc":
            vcc = 0 if op.startswith("v_cmp_lt_u32") else None
        elif re.match(r"s_\w+_b64$", op) and s[len(op):].split(",")[0].strip() == "vcc":
            vcc = None
        if op.startswith("s_cbranch") or op == "s_branch":
            tgt = s.split()[-1]
            if op == "s_branch":
                taken = True
            elif tgt == header:
                taken = True
            elif op in ("s_cbranch_scc0", "s_cbranch_scc1") and scc is not None:
                taken = (scc == 1) == (op == "s_cbranch_scc1")
            elif op in ("s_cbranch_vccz", "s_cbranch_vccnz") and vcc is not None:
                taken = (vcc == 0) == (op == "s_cbranch_vccz")
            elif op in ("s_cbranch_execz", "s_cbranch_execnz"):
                taken = op == "s_cbranch_execnz"
            elif tgt not in in_loop:
                taken = False  # a way out of the loop
            else:
                taken = False
                notes.append(f"undecided branch assumed not taken: {s}")
            path.append((i, s, taken))
            if taken:
                if tgt == header:
                    break
                i = labels[tgt]
                continue
        else:
            path.append((i, s, None))
        i += 1
    else:
        notes.append("gave up after 4000 lines")
    return path, notes


def census(path):
    c = dict(filter_valu=0, other_valu=0, salu=0, smem=0, waits=0, nops=0, branches=0, taken=0)
    other = []
    for _, s, taken in path:
        op = s.split()[0]
        if op.startswith(FILTER):
            c["filter_valu"] += 1
        elif op.startswith("v_"):
            c["other_valu"] += 1
            other.append(s)
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            c["smem"] += 1
        elif op == "s_waitcnt":
            c["waits"] += 1
        elif op == "s_nop":
            c["nops"] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            c["branches"] += 1
            c["taken"] += 1 if taken else 0
        else:
            c["salu"] += 1
    c["total"] = len(path)
    # distance from every load to the wait that retires it, around the loop
    dist = []
    n = len(path)
    for k, (_, s, _) in enumerate(path):
        if not s.startswith("s_load"):
            continue
        ins = valu = 0
        for step in range(1, n + 1):
            t = path[(k + step) % n][1]
            if t.startswith("s_waitcnt") and "lgkmcnt" in t:
                break
            ins += 1
            valu += 1 if t.split()[0].startswith(FILTER) else 0
        dist.append((s, ins, valu))
    return c, other, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "raytracinginoneweekendincuda_amd", "csrc", "render.hip"))
    ap.add_argument("--label", default="")
    ap.add_argument("--keep", default=None, help="keep the assembly files in this directory")
    args = ap.parse_args()
    keep = args.keep or tempfile.mkdtemp(prefix="scan_census_")
    os.makedirs(keep, exist_ok=True)
    print(f"== packed-filter loops of the sphere-list kernel{': ' + args.label if args.label else ''} ==")
    for build in ("strict", "fast"):
        lines = assemble(os.path.abspath(args.src), build, keep)
        for name, lo, hi in functions(lines):
            headers = []
            for i in range(lo, hi):
                m = LABEL.match(lines[i])
                # (the label's own comment block: one "Parent Loop" line per level of nesting, then the header's)
                j = i + 1
                while j < hi and "Parent Loop" in lines[j] and not LABEL.match(lines[j]):
                    j += 1
                if m and i + 1 < hi and "Loop Header" in " ".join(lines[i:j + 1]):
                    headers.append(m.group(1))
            for header in headers:
                path, notes = quiet_trip(lines, lo, hi, header, headers)
                if path is None:
                    continue
                on_rows = sum(1 for _, s, _ in path if s.startswith(("v_pk_mul_f32", "v_pk_fma_f32")) and re.search(r"\bs\[\d+:\d+\]", s))
                pk_mul = sum(1 for _, s, _ in path if s.startswith("v_pk_mul_f32") and re.search(r"\bs\[\d+:\d+\]", s))
                pairs = sum(1 for _, s, _ in path if SQUARE.match(s))
                if not on_rows or not pairs or not any(s.startswith("s_load_dwordx8") for _, s, _ in path):
                    continue
                form = "general" if pk_mul else "run"
                c, other, dist = census(path)
                regs = next((ln.split()[-1] for ln in lines[lo:hi + 400] if ".amdhsa_next_free_vgpr" in ln), "?")
                scratch = next((ln.split()[-1] for ln in lines[lo:hi + 400] if ".amdhsa_private_segment_fixed_size" in ln), "?")
                m = re.search(r"TraitsILi(\d)", name)
                print(f"\n{build} build, kernel ...Traits<{m.group(1) if m else '?'},...> ({regs} VGPRs, {scratch} B scratch), {form} loop {header}: "
                      f"{2 * pairs} spheres per trip")
                print(f"  quiet trip: {c['total']} instructions = {c['filter_valu']} filter VALU + {c['other_valu']} other VALU + {c['salu']} SALU + "
                      f"{c['smem']} SMEM + {c['waits']} waits + {c['nops']} s_nop + {c['branches']} branches ({c['taken']} taken)")
                for s in other:
                    print(f"    other VALU: {s}")
                for s, ins, valu in dist:
                    print(f"    {s:<58} -> its wait: {ins:3d} instructions later, {valu:2d} of them filter VALU")
                for n_ in notes:
                    print(f"    note: {n_}")


if __name__ == "__main__":
    sys.exit(main())
