#!/usr/bin/env python3
"""Compare the instruction streams of the kernels in two device assembly files (hipcc --cuda-device-only -S).

    python tools/isa_compare.py parent.s change.s [name-substring] [old=new ...]

Each file is split at its kernel labels; comments, directives and blank lines are dropped, and what remains of each kernel
(instructions and local labels) is compared text for text; a local label .LBB<f>_<n> is read without <f>, the position of its
function in the file, which moves when a function is added or removed above it.  For a kernel that differs the differing
lines and the counts of the instructions that make up a pipeline stage are printed.  Exit status 0: the same kernels, every one identical.

Kernels are paired by their mangled names.  Where a change renamed a kernel or gave it other template or function parameters,
each argument old=new replaces the substring `old` by `new` in the names of the FIRST file before the pairing, e.g.
17knn_groups_kernel=17knn_search_kernel; without such arguments names are compared as they are."""
import difflib
import re
import sys

COUNTED = [("mfma", r"^v_mfma"), ("ds_read_b128", r"^ds_read_b128"), ("lds-dma", r"^buffer_load_dword.*\blds\b"),
           ("s_barrier", r"^s_barrier"), ("s_waitcnt", r"^s_waitcnt")]


def kernels(path, want):
    out, name, body = {}, None, None
    kernel_names = set()
    with open(path) as f:
        lines = f.read().splitlines()
    for line in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernel_names.add(m.group(1))
    for line in lines:
        m = re.match(r"(\w+):", line)
        if m and m.group(1) in kernel_names:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            if want in name:
                out[name] = body
            name = None
            continue
        text = line.split(";")[0].strip()
        if text and not (text.startswith(".") and not text.endswith(":")):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", text)))
    return out


def counts(body):
    return {key: sum(1 for line in body if re.match(rx, line)) for key, rx in COUNTED}


def main():
    renames = [arg.split("=", 1) for arg in sys.argv[3:] if "=" in arg]
    want = next((arg for arg in sys.argv[3:] if "=" not in arg), "")
    a, b = kernels(sys.argv[1], ""), kernels(sys.argv[2], want)
    for old, new in renames:
        a = {name.replace(old, new): body for name, body in a.items()}
    a = {name: body for name, body in a.items() if want in name}
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"ONLY IN {'first' if name in a else 'second'}: {name}")
            bad += 1
        elif a[name] != b[name]:
            bad += 1
            print(f"DIFFERS: {name}\n  first:  {len(a[name])} lines {counts(a[name])}\n  second: {len(b[name])} lines {counts(b[name])}")
            sys.stdout.write("\n".join(difflib.unified_diff(a[name], b[name], "first", "second", n=0, lineterm="")) + "\n")
    print(f"{len(a)} / {len(b)} kernels, {len(set(a) & set(b)) - sum(1 for n in set(a) & set(b) if a[n] != b[n])} identical, {bad} not")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
