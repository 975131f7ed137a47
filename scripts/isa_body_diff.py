#!/usr/bin/env python3
"""Compare the instruction bodies of kernels between two `hipcc --cuda-device-only -S` listings (e.g. blend.hip before and
after a change, built with tests/test_isa_guards.py's flags).  Symbol names, local labels and comments are normalised away,
so a kernel whose template argument was renamed still compares; the kernel descriptor is compared too.

    python scripts/isa_body_diff.py before.s after.s OLD_SUBSTRING=NEW_SUBSTRING [...]
    e.g. k_blend_linearILb0E=k_blend_linearILi0E k_gain_overlap=k_gain_overlap
    python scripts/isa_body_diff.py --by-name before.s [...] -- after.s [...]
    every kernel of the first listings against the kernel of the same demangled name (anonymous namespaces dropped) in the
    second ones: a move of kernels between files, as blend.hip -> blend.hip, overlap.hip, canvas.hip
Exit status 1 when an instruction differs, or with --by-name when a kernel is missing or the counts differ."""
import difflib
import re
import subprocess
import sys


def bodies(path):
    out, cur = {}, None
    for line in open(path).read().split("\n"):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur = m.group(1); out[cur] = []; continue
        if cur:
            if line.startswith(".Lfunc_end"):
                cur = None; continue
            out[cur].append(line)
    return out


def norm(lines, name):
    return [re.sub(r"\s*;.*$", "", re.sub(r"\.L\w+", ".L", l.replace(name, "SYM"))) for l in lines if not l.strip().startswith(";")]


def plain_names(symbols):
    """symbol -> its demangled name without anonymous-namespace qualifiers: what a kernel keeps when it, or the type of an
    argument, moves between translation units."""
    symbols = list(symbols)
    out = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    return {s: d.replace("(anonymous namespace)::", "") for s, d in zip(symbols, out)}


def main():
    if sys.argv[1] == "--by-name":
        # every kernel of the listings before "--" against the kernel of that name in the listings after it
        cut = sys.argv.index("--")
        before, after = {}, {}
        def kernels(p):          # the functions among the labels (a __constant__ table has a mangled label too)
            funcs = set(re.findall(r"^\s*\.type\s+(_Z\S+),@function", open(p).read(), re.M))
            return {k: v for k, v in bodies(p).items() if k in funcs}
        for p in sys.argv[2:cut]:
            before.update(kernels(p))
        for p in sys.argv[cut + 1:]:
            after.update(kernels(p))
        nb, na = plain_names(before), plain_names(after)
        by_name = {d: s for s, d in na.items()}
        pairs = [(nb[s], s, by_name.get(nb[s])) for s in before]
        print(f"{len(before)} kernels before, {len(after)} after")
        bad = len(before) != len(after)
    else:
        before, after = bodies(sys.argv[1]), bodies(sys.argv[2])
        bad = False
        pairs = []
        for spec in sys.argv[3:]:
            old, new = spec.split("=")
            nb = [k for k in before if old in k]; na = [k for k in after if new in k]
            if len(nb) != 1 or len(na) != 1:
                print(f"{spec}: {len(nb)} / {len(na)} matching symbols"); bad = True; continue
            pairs.append((spec, nb[0], na[0]))
    for spec, sb, sa in pairs:
        if sa is None:
            print(f"{spec}: no kernel of this name after"); bad = True; continue
        x, y = norm(before[sb], sb), norm(after[sa], sa)
        diff = [l for l in difflib.unified_diff(x, y, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        code = [l for l in diff if not l[1:].strip().startswith(".")]
        print(f"{spec}: {len(x)} lines, {'identical instructions' if not code else 'INSTRUCTIONS DIFFER'}"
              + (f"; directives: {' | '.join(d.strip() for d in diff if d not in code)}" if diff and not code else ""))
        for l in code[:20]:
            print("   ", l)
        bad |= bool(code)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
