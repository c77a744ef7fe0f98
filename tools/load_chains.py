#!/usr/bin/env python3
"""Dependent load chains of the kernels of one source file, read from the generated gfx950 code.

Usage:  python tools/load_chains.py csrc-file.hip [kernel-name-substring ...] [-D...]

Compiles the file with the product flags of 3dgs-avatar-release_amd/build.py plus `--cuda-device-only -S` (no GPU
needed) and prints, per kernel, in program order: the vector memory loads (runs of loads with no wait between them on
one line), the `s_waitcnt vmcnt(n)` waits with their counts, the workgroup barriers and the loop heads (labels that a
later branch jumps back to) with the branches that close them.  A full wait -- vmcnt(0) -- between two runs of loads
that do not depend on each other is a round trip the data flow does not need.  The kernel's header line carries its
VGPR count and scratch bytes, since a change that puts more loads in flight pays in registers.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3dgs-avatar-release_amd"))
import build as product  # noqa: E402  (the flags, the strict list and the compiler come from the product build)

LOAD = re.compile(r"^\s+((?:global|flat|buffer|scratch)_load_\w+)\s")
WAIT = re.compile(r"^\s+s_waitcnt\s+(.*?)\s*(?:;.*)?$")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
FUNC = re.compile(r"^([A-Za-z_][\w$.]*):")
META = re.compile(r"^\s+\.amdhsa_(next_free_vgpr|private_segment_fixed_size|group_segment_fixed_size)\s+(\d+)")


def assembly(src, extra):
    name = os.path.basename(src)
    flags = list(product.COMMON) + (["-ffp-contract=off"] if name in product.STRICT else ["-ffp-contract=fast"])
    if name in product.NO_SLP:
        flags.append("-fno-slp-vectorize")
    cmd = [product.hipcc()] + flags + extra + ["--cuda-device-only", "-S", src, "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed:\n" + r.stderr)
    return r.stdout.splitlines()


def kernels(lines):
    """(name, body lines, {meta}) of every kernel: a body runs from the kernel's label to its s_endpgm-terminated end."""
    names = [m.group(1) for m in (re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    meta, cur = {}, None
    for ln in lines:
        m = re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = meta.setdefault(m.group(1), {})
        elif cur is not None:
            m = META.match(ln)
            if m:
                cur[m.group(1)] = int(m.group(2))
            elif ".end_amdhsa_kernel" in ln:
                cur = None
    out, i = [], 0
    while i < len(lines):
        m = FUNC.match(lines[i])
        if m and m.group(1) in names:
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            out.append((m.group(1), lines[i + 1:j], meta.get(m.group(1), {})))
            i = j
        i += 1
    return out


def chain(body):
    seen, heads = {}, set()
    for n, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            seen[m.group(1)] = n
        m = BRANCH.match(ln)
        if m and m.group(1) in seen:
            heads.add(m.group(1))
    events, run = [], []

    def flush():
        if run:
            events.append("  load x%-2d %s" % (len(run), " ".join(s.split("_load_")[1] for s in run)))
            del run[:]

    for n, ln in enumerate(body):
        m = LOAD.match(ln)
        if m:
            run.append(m.group(1))
            continue
        m = WAIT.match(ln)
        if m:
            v = VMCNT.search(m.group(1))
            if v:
                flush()
                events.append("  wait vmcnt(%s)" % v.group(1))
            continue
        if re.match(r"^\s+s_barrier\b", ln):
            flush()
            events.append("  barrier")
            continue
        m = LABEL.match(ln)
        if m and m.group(1) in heads:
            flush()
            events.append(" loop %s:" % m.group(1))
            continue
        m = BRANCH.match(ln)
        if m and m.group(1) in heads and seen[m.group(1)] < n:
            flush()
            events.append("  back to %s" % m.group(1))
    flush()
    return events


def demangle(names):
    for tool in ("llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool] + names, capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0 and len(r.stdout.splitlines()) == len(names):
            return [re.sub(r"^void ", "", s.split("(")[0]) for s in r.stdout.splitlines()]
    return names


def main(argv):
    extra = [a for a in argv if a.startswith("-D")]
    args = [a for a in argv if not a.startswith("-D")]
    if not args:
        sys.exit(__doc__)
    src = args[0] if os.path.exists(args[0]) else os.path.join(product.CSRC, args[0])
    ks = kernels(assembly(src, extra))
    pretty = demangle([k[0] for k in ks])
    for (name, body, meta), shown in zip(ks, pretty):
        if args[1:] and not any(p in shown for p in args[1:]):
            continue
        print("%s  vgpr=%s scratch=%s lds=%s" % (shown, meta.get("next_free_vgpr", "?"), meta.get("private_segment_fixed_size", "?"),
                                              meta.get("group_segment_fixed_size", "?")))
        for ev in chain(body):
            print(ev)
        print()


if __name__ == "__main__":
    main(sys.argv[1:])
