"""Compares the device assembly of two builds of one .hip file kernel by kernel, whatever the order of emission.

usage: python tools/isa_by_kernel.py PARENT.s BRANCH.s     (each from hipcc ... --cuda-device-only -S -cuid=NAME FILE.hip)

The compiler emits kernels in the order the host code first names them, numbers labels (.LBB<n>_, .Lfunc_end<n>) and
loop-header comments by that order and pads a label's comment to a column; a launcher that names the same instantiations
elsewhere therefore gives another file with the same kernels. This splits both files at the kernels' sections and their
metadata entries, replaces the mangled soc:: symbols and those order-dependent numbers, drops the trailer after the last kernel, sorts by demangled name (the
anonymous namespace dropped) and compares each kernel's text and its metadata entry (registers, LDS, kernarg layout).
One line per kernel with a hash; exit status 1 when a kernel differs or the sets differ."""
import hashlib
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::", "", o) for o in out[:len(names)]]


def norm(text):
    text = re.sub(r"_ZN3soc[A-Za-z0-9_.$]*", "SOC_SYMBOL", text)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"Header=BB\d+_", "Header=BB_", text)   # the function's index in comments
    text = re.sub(r"(Child|Parent) Loop BB\d+_", r"\1 Loop BB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    return re.sub(r"(?m)^(\.LBB_\d+:)[ \t]+;", r"\1 ;", text)   # the comment column follows the label's width


def split(path):
    lines = open(path).read().split("\n")
    meta = next(i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata")
    body, md = lines[:meta], lines[meta:]
    starts, syms = [], []
    for i, l in enumerate(body):
        m = re.match(r"\t\.section\t\.text\.(_Z\w+),", l)
        if m and m.group(1) not in syms:
            starts.append(i)
            syms.append(m.group(1))
    chunks = {}
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(body)
        # the kernel emitted last carries the file's trailer (the code's end padding, register maximums, the cuid object)
        chunks[syms[k]] = re.split(r"\n(?:\t\.text\n\t\.p2alignl 6, \d+\n\t\.fill 256, 4, \d+\n)?\t\.section\t\.AMDGPU\.gpr_maximums", "\n".join(body[s:e]))[0]
    head = "\n".join(body[:starts[0]])
    # metadata entries: each starts at "  - .agpr_count:" (first key of a kernel entry, keys sorted)
    ms = [i for i, l in enumerate(md) if re.match(r"  - \.\w+", l)]
    mchunks = {}
    for k, s in enumerate(ms):
        e = ms[k + 1] if k + 1 < len(ms) else len(md)
        ent = md[s:e]
        name = next(re.search(r"(_Z\w+)", l).group(1) for l in ent if ".name:" in l and "_Z" in l)
        # the last entry carries the file's trailer
        mchunks[name] = "\n".join(ent).split("\namdhsa.target:")[0]
    names = demangle(syms)
    out = {}
    for sym, n in zip(syms, names):
        out[n] = (norm(chunks[sym]), norm(mchunks[sym]))
    return out, norm(head), names


a, ha, na = split(sys.argv[1])
b, hb, nb = split(sys.argv[2])
print("kernels:", len(a), len(b), "same set:", sorted(a) == sorted(b), "same order:", na == nb, "same head:", ha == hb)
bad = 0
for n in sorted(a):
    ta, ma = a[n]
    tb, mb = b.get(n, ("", ""))
    ok_t, ok_m = ta == tb, ma.split("\n...")[0] == mb.split("\n...")[0]
    if not (ok_t and ok_m):
        bad += 1
    print("%s %s  text %s  %5d lines  %s" % ("OK " if ok_t and ok_m else "DIFF", hashlib.sha256((ta + ma.split("\n...")[0]).encode()).hexdigest()[:16],
                                           "same" if ok_t else "DIFF", ta.count("\n") + 1, n.split("(")[0]))
print("differing kernels:", bad)
h = lambda d: hashlib.sha256("\n".join(d[n][0] + d[n][1].split("\n...")[0] for n in sorted(d)).encode()).hexdigest()
print("sha256 over the kernels sorted by demangled name:", h(a), h(b))
sys.exit(1 if bad or sorted(a) != sorted(b) else 0)
