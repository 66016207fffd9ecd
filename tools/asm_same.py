#!/usr/bin/env python3
"""Are two device assembly files (hipcc --cuda-device-only -S, e.g. `make asm` of two trees) the same code?

    python3 tools/asm_same.py [-q] A.s B.s

The files are split by function symbol.  Per symbol the instruction stream, the .amdhsa_* directives of its kernel
descriptor, its `.set <symbol>.*` resource lines and its entry in the amdhsa.kernels metadata are compared as text,
after comments are dropped and the local labels whose numbers depend on a function's position in the file or on
unrelated code (.LBB<n>_, .Lpost_getpc, .Ltmp, .Lfunc_end) are renumbered per symbol.  Prints identical / different
per symbol (with the first differing line) and exits non-zero on any difference or on a symbol only one file has.
"""
import re
import sys

SYM = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.L(BB)\d+_(\d+)|\.L(post_getpc|tmp|func_end)(\d+)")


def clean(line):
    return line.split(";", 1)[0].strip()


def normalise(lines):
    seen = {}

    def sub(m):
        if m.group(1):
            return ".LBB_" + m.group(2)
        key = (m.group(3), m.group(4))
        if key not in seen:
            seen[key] = sum(1 for k in seen if k[0] == m.group(3))
        return ".L%s#%d" % (m.group(3), seen[key])

    return [LOCAL.sub(sub, ln) for ln in lines]


def functions(text):
    """symbol -> cleaned lines from its label to its .Lfunc_end, plus its .set lines"""
    out, cur, sym = {}, None, None
    for raw in text.splitlines():
        ln = clean(raw)
        if not ln:
            continue
        m = SYM.match(ln)
        if cur is None:
            if m and not ln.startswith(".L"):
                sym, cur = m.group(1), []
            elif ln.startswith(".set ") and ln[5:].split(",")[0].rsplit(".", 1)[0] in out:
                out[ln[5:].split(",")[0].rsplit(".", 1)[0]].append(ln)
            continue
        cur.append(ln)
        if ln.startswith(".Lfunc_end"):
            out[sym] = cur
            cur = None
    return {s: normalise(v) for s, v in out.items()}


def metadata(text):
    """kernel name -> lines of its amdhsa.kernels entry"""
    out = {}
    i = text.find("amdhsa.kernels:")
    if i < 0:
        return out
    item = []
    for raw in text[i:].splitlines()[1:]:
        if raw.startswith("  - ") or not raw.startswith("  "):
            if item:
                name = [ln.split(":", 1)[1].strip() for ln in item if ln.strip().startswith(".name:")]
                out[name[0].strip("'\"")] = item
            item = []
            if not raw.startswith("  "):
                break
        item.append(raw.rstrip())
    return out


def first_diff(a, b):
    for n, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %r != %r" % (n, x, y)
    return "lengths %d != %d" % (len(a), len(b))


def main(pa, pb, quiet=False):
    ta, tb = open(pa).read(), open(pb).read()
    fa, fb, ma, mb = functions(ta), functions(tb), metadata(ta), metadata(tb)
    bad = 0
    for s in sorted(set(fa) | set(fb)):
        kind = "kernel" if s in ma or s in mb else "function"
        if s not in fa or s not in fb:
            print("only in %s  %s %s" % (pa if s in fa else pb, kind, s))
            bad += 1
        elif fa[s] != fb[s]:
            print("different  %s %s  code, %s" % (kind, s, first_diff(fa[s], fb[s])))
            bad += 1
        elif ma.get(s) != mb.get(s):
            print("different  %s %s  metadata, %s" % (kind, s, first_diff(ma.get(s) or [], mb.get(s) or [])))
            bad += 1
        elif not quiet:
            print("identical  %s %s  (%d lines)" % (kind, s, len(fa[s])))
    print("%s vs %s: %d symbols, %d kernels, %d differ" % (pa, pb, len(set(fa) | set(fb)), len(set(ma) | set(mb)), bad))
    return 1 if bad or not fa else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-q"]   # -q: only the symbols that differ, and the summary line
    if len(args) != 2:
        raise SystemExit(__doc__)
    sys.exit(main(args[0], args[1], quiet=len(args) < len(sys.argv) - 1))
