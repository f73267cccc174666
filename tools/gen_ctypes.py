#!/usr/bin/env python3
"""Generate dostransformer_amd/_abi.py from include/dosx.h: the ctypes side of the C ABI.

One ctypes.Structure per `typedef struct DosxX { ... } DosxX;` (named X, fields in header order), SIGS / RESTYPES for every
`dosx_*` prototype, and every enumerator / integer `#define DOSX_*` as a module-level int.  The ctypes type is a function of
the declared C type alone; a declaration outside the header's closed set of types stops the generator with its line - it
never guesses.  Run by the Makefile whenever dosx.h changes; the output is deterministic (header order) and committed.

usage: gen_ctypes.py <include/dosx.h> <out.py>"""
import re
import sys

from gen_replay_thunks import declarations, strip_comments

SCALARS = {"int": "C.c_int", "int32_t": "C.c_int32", "int64_t": "C.c_int64", "long long": "C.c_int64", "size_t": "C.c_size_t",
           "float": "C.c_float", "double": "C.c_double"}
POINTEES = set(SCALARS) | {"void", "unsigned long long"}       # a pointer to any of these is an address: c_void_p


class Unmapped(ValueError):
    """A declaration outside the closed set; `pos` is its offset in the comment-free header (None: the caller's)."""

    def __init__(self, what, pos=None):
        super().__init__(what)
        self.pos = pos


def ctype(ty, structs, by_value):
    """ctypes expression of one declared C type; by_value: a struct field (nested structs allowed), else a parameter."""
    t = " ".join(re.sub(r"\bconst\b", " ", ty).replace("*", " * ").split())
    if t in SCALARS:
        return SCALARS[t]
    if t == "dosx_stream_t" and not by_value:
        return "C.c_void_p"
    if t.endswith(" *"):
        base = t[:-2]
        if base in POINTEES:
            return "C.c_void_p"
        if base == "char":
            return "C.c_char_p"
        if base in structs and not by_value:
            return f"C.POINTER({base[4:]})"
    elif t in structs and by_value:
        return t[4:]
    raise Unmapped(f"type `{ty}`")


def fields(body, pos0, structs):
    """[(name, ctypes expression)] of a struct body: `type a, b;`, `type* p;`, `type a[3];` - anything else is refused."""
    out = []
    for d in re.finditer(r"[^;]*[^;\s][^;]*", body):
        decl, pos = " ".join(d.group(0).split()), pos0 + d.start() + len(d.group(0)) - len(d.group(0).lstrip())
        m = re.match(r"^((?:const )?(?:unsigned )?(?:long long|\w+) ?\*?) ?(\w+(?:\[\w*\])?(?: ?, ?\w+(?:\[\w*\])?)*)$", decl)
        if not m:
            raise Unmapped(f"declaration `{decl}`", pos)
        names = [n.strip() for n in m.group(2).split(",")]
        if "*" in m.group(1) and len(names) > 1:
            raise Unmapped(f"declaration `{decl}` (one pointer per declaration)", pos)
        try:
            ct = ctype(m.group(1), structs, True)
        except Unmapped as e:
            raise Unmapped(f"{e} of field `{decl}`", pos) from None
        for n in names:
            a = re.match(r"^(\w+)\[(\w*)\]$", n)
            if a and not a.group(2).isdigit():
                raise Unmapped(f"array size of `{decl}` (not a literal)", pos)
            out.append((a.group(1), f"{ct} * {a.group(2)}") if a else (n, ct))
    return out


def parse(text):
    """(items, sigs, restypes) of the comment-free header; items = (offset, kind, payload) of structs and constants."""
    items, structs, keywords = [], [], []
    for m in re.finditer(r"\btypedef\s+(struct)\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        if m.group(2) != m.group(4) or not m.group(2).startswith("Dosx") or re.search(r"[{}]", m.group(3)):
            raise Unmapped(f"struct `{m.group(2)}` (not `typedef struct DosxX {{ fields }} DosxX;`)", m.start())
        items.append((m.start(), "struct", (m.group(2)[4:], fields(m.group(3), m.start(3), structs))))
        structs.append(m.group(2))
        keywords.append(m.start(1))
    for m in re.finditer(r"\b(?:struct|union)\b", text):
        if m.start() not in keywords:
            raise Unmapped(f"`{m.group(0)}` (not `typedef struct DosxX {{ fields }} DosxX;`)", m.start())
    for m in re.finditer(r"\benum\b\s*\w*\s*\{(.*?)\}", text, flags=re.S):
        for e in m.group(1).split(","):
            mm = re.match(r"^\s*(DOSX_\w+)\s*=\s*(-?\d+)\s*$", e)
            if e.strip() and not mm:
                raise Unmapped(f"enumerator `{' '.join(e.split())}` (not `DOSX_X = integer`)", m.start())
            if mm:
                items.append((m.start(), "const", (mm.group(1), int(mm.group(2)))))
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(DOSX_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M):
        items.append((m.start(), "const", (m.group(1), int(m.group(2)))))
    sigs, restypes = [], []
    for ret, name, params, pos in declarations(text):
        try:
            sigs.append((name, [ctype(p, structs, False) for p in params]))
            if ret != "int":
                restypes.append((name, ctype(ret, structs, False)))
        except Unmapped as e:
            raise Unmapped(f"{e} in the prototype of `{name}`", pos) from None
    for m in re.finditer(r"\bdosx_\w+(?=\s*\()", text):
        if m.group(0) not in dict(sigs):
            raise Unmapped(f"`{m.group(0)}(` (not a prototype the scan understands)", m.start())
    return items, sigs, restypes


def generate(header):
    """The text of _abi.py for the header text; Unmapped, with the header's line, for a declaration outside the closed set."""
    text = strip_comments(header)
    try:
        items, sigs, restypes = parse(text)
    except Unmapped as e:
        n = text.count("\n", 0, e.pos) + 1
        raise Unmapped(f"dosx.h:{n}: cannot map {e}\n    {header.splitlines()[n - 1].strip()}") from None

    out = ["# GENERATED by tools/gen_ctypes.py from include/dosx.h — do not edit.",
           "# ctypes mirrors of the header's structs, argtypes / restypes of its entry points, and its integer constants.",
           "import ctypes as C", ""]
    for _, kind, (name, val) in sorted(items, key=lambda it: it[0]):     # stable: enumerators of one enum keep their order
        if kind == "const":
            out.append(f"{name} = {val}")
        else:
            out += ["", "", f"class {name}(C.Structure):", "    _fields_ = ["]
            out += [f'        ("{f}", {t}),' for f, t in val]
            out += ["    ]", "", ""]
    out += ["", "# name -> argtypes", "SIGS = {"]
    out += [f'    "{name}": [{", ".join(args)}],' for name, args in sigs]
    out += ["}", "", "# restype where it is not int", "RESTYPES = {"]
    out += [f'    "{name}": {t},' for name, t in restypes]
    out += ["}", ""]
    return re.sub(r"\n{4,}", "\n\n\n", "\n".join(out))


def main():
    src, dst = sys.argv[1:3]
    try:
        text = generate(open(src).read())
    except Unmapped as e:
        sys.exit(f"gen_ctypes.py: {e}")
    open(dst, "w").write(text)


if __name__ == "__main__":
    main()
