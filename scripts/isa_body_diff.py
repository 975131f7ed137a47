#!/usr/bin/env python3
"""Compare the instruction bodies of kernels between two `hipcc --cuda-device-only -S` listings (e.g. blend.hip before and
after a change, built with tests/test_isa_guards.py's flags).  Symbol names, local labels and comments are normalised away,
so a kernel whose template argument was renamed still compares; the kernel descriptor is compared too.

    python scripts/isa_body_diff.py before.s after.s OLD_SUBSTRING=NEW_SUBSTRING [...]
    e.g. k_blend_linearILb0E=k_blend_linearILi0E k_gain_overlap=k_gain_overlap
Exit status 1 when an instruction differs."""
import difflib
import re
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


def main():
    before, after = bodies(sys.argv[1]), bodies(sys.argv[2])
    bad = False
    for spec in sys.argv[3:]:
        old, new = spec.split("=")
        nb = [k for k in before if old in k]; na = [k for k in after if new in k]
        if len(nb) != 1 or len(na) != 1:
            print(f"{spec}: {len(nb)} / {len(na)} matching symbols"); bad = True; continue
        x, y = norm(before[nb[0]], nb[0]), norm(after[na[0]], na[0])
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
