"""CPU-only checks of the C-ABI boundary: libdosx.so loads and exports every symbol include/dosx.h declares; the GENERATED
binding (dostransformer_amd/_abi.py, tools/gen_ctypes.py) is checked against the header as a whole - every field of every struct
with a gcc-compiled probe of the real header, every argument of every prototype, every constant.  No compute calls (there is no
GPU here)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dosx.h")


def _gen(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def _code():
    """include/dosx.h without its comments."""
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S))


def _declared():
    return sorted(set(re.findall(r"\b(dosx_[a-z0-9_]+)\s*\(", _code())))


def _structs():
    """[(C name, [(field type, field name, array length or None)])] of every struct of the header, parsed here (not by the generator)."""
    out = []
    for name, body in re.findall(r"typedef struct (Dosx\w+) \{(.*?)\} \1;", _code(), flags=re.S):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            ty, first = re.match(r"^(.*?)(\w+(?:\[\d+\])?(?: ?, ?\w+(?:\[\d+\])?)*)$", decl).groups()
            for n in first.split(","):
                m = re.match(r"^ ?(\w+)(?:\[(\d+)\])?$", n)
                fields.append((ty.strip(), m.group(1), int(m.group(2)) if m.group(2) else None))
        out.append((name, fields))
    return out


def _header_constants():
    """{name: value} of every enumerator and integer #define DOSX_* of the header, parsed here (not by the generator)."""
    code, out = _code(), {}
    for body in re.findall(r"\benum\s*\{(.*?)\}", code, flags=re.S):
        for name, val in re.findall(r"(DOSX_\w+)\s*=\s*(-?\d+)", body):
            out[name] = int(val)
        assert len(re.findall(r"DOSX_\w+", body)) == body.count("=") == len([e for e in body.split(",") if e.strip()])
    for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DOSX_\w+)[ \t]+(-?\d+)[ \t]*$", code, flags=re.M):
        out[name] = int(val)
    return out


# C type -> (sizeof, class) on the one ABI the library is built for (LP64); the probe below confirms the sizes with gcc.
# Independent of tools/gen_ctypes.py on purpose: what the binding declares is compared with what the HEADER declares.
SCALARS = {"int": (4, "int"), "int32_t": (4, "int"), "int64_t": (8, "int"), "long long": (8, "int"), "unsigned long long": (8, "uint"),
           "size_t": (8, "uint"), "float": (4, "float"), "double": (8, "float")}
CODES = {"int": "bhilq", "uint": "BHILQ", "float": "fd"}         # ctypes' one-letter type codes per class


def _assert_ctype(ct, c_type, by_value, where):
    """``ct`` (a ctypes type) is what the declared C type asks for: scalar class and size, pointer-ness, which struct."""
    from dostransformer_amd import _abi
    t = " ".join(re.sub(r"\bconst\b", " ", c_type).replace("*", " * ").split())
    if t.endswith(" *"):
        base = t[:-2]
        if base == "char":
            assert ct is C.c_char_p, where
        elif base.startswith("Dosx"):
            assert not by_value and ct is C.POINTER(getattr(_abi, base[4:])) and ct._type_.__name__ == base[4:], where
        else:
            assert base in SCALARS or base == "void", where
            assert ct is C.c_void_p, where
    elif t == "dosx_stream_t":
        assert not by_value and ct is C.c_void_p, where
    elif t.startswith("Dosx"):
        assert by_value and ct is getattr(_abi, t[4:]), where
    else:
        size, cls = SCALARS[t]
        assert isinstance(getattr(ct, "_type_", None), str) and ct._type_ in CODES[cls] and C.sizeof(ct) == size, (where, ct)


def test_library_exports_every_declared_symbol():
    from tests.util import dosx_lib
    _lib = dosx_lib()
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/dosx.h but not exported by libdosx.so"
    assert set(names) == set(_lib.EXPORTS), set(names) ^ set(_lib.EXPORTS)
    assert lib.dosx_version() >= 100


def test_ctypes_structs_match_c_layout(tmp_path):
    """THE check of the whole boundary's data side: one gcc probe over every field of every struct of include/dosx.h.  Each
    ctypes mirror has the header's field names in the header's order, every field its C offset, size and type class, every
    struct its C size."""
    from dostransformer_amd import _abi, _lib
    structs = _structs()
    mirrors = {k: v for k, v in vars(_abi).items() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert len(structs) >= 24 and {n[4:] for n, _ in structs} == set(mirrors)
    assert len(structs) == len(re.findall(r"\b(?:struct|union)\b", _code()))           # no struct the regex above missed
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dosx.h"', "int main(void) {"]
    lines += [f'  printf("%zu\\n", sizeof({t}));' for t in SCALARS]
    for name, fields in structs:
        lines.append(f'  printf("%zu\\n", sizeof({name}));')
        lines += [f'  printf("%zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for _, f, _ in fields]
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert [int(next(out)) for _ in SCALARS] == [size for size, _ in SCALARS.values()]
    for name, fields in structs:
        cls = mirrors[name[4:]]
        assert getattr(_lib, name[4:]) is cls                                           # re-exported under the same name
        assert [f for f, _ in cls._fields_] == [f for _, f, _ in fields], name
        assert C.sizeof(cls) == int(next(out)), name
        for (c_type, f, n), (_, ct) in zip(fields, cls._fields_):
            d = getattr(cls, f)
            assert [d.offset, d.size] == [int(v) for v in next(out).split()], (name, f)
            if n is not None:
                assert issubclass(ct, C.Array) and ct._length_ == n, (name, f)
                ct = ct._type_
            _assert_ctype(ct, c_type, True, (name, f))
    assert next(out, None) is None


def test_argtypes_and_restypes_match_the_header_prototypes():
    """THE check of the boundary's call side: for every prototype of include/dosx.h the loaded function's argtypes have the
    prototype's arity and, argument by argument, its class (integer / floating point / address / descriptor pointer / string),
    scalar size and descriptor type; restype likewise.  The expectation is computed here from the header text."""
    from tests.util import dosx_lib
    lib = dosx_lib().load()
    gen = _gen("gen_replay_thunks")
    decls = list(gen.declarations(gen.strip_comments(open(HEADER).read())))
    assert [d[1] for d in decls] == list(dosx_lib().EXPORTS) and sorted(d[1] for d in decls) == _declared() and len(decls) >= 125
    n_struct = 0
    for ret, name, params, _ in decls:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params), name
        for i, (ct, c_type) in enumerate(zip(fn.argtypes, params)):
            _assert_ctype(ct, c_type, False, (name, i, c_type))
            n_struct += "Dosx" in c_type
        _assert_ctype(fn.restype, ret, False, (name, "return"))
    assert n_struct == len(re.findall(r"\bconst Dosx\w+\s*\*", _code())) >= 32       # every descriptor pointer was seen as one
    # spot facts straight from the header, so that the walk above cannot pass by checking nothing
    assert lib.dosx_adamw_f64.argtypes[5] is C.c_double and lib.dosx_adamw.argtypes[5] is C.c_float
    assert lib.dosx_softmax_fwd.argtypes[2] is C.c_int64 and lib.dosx_csr_build.argtypes[17] is C.c_size_t
    assert lib.dosx_last_error.restype is C.c_char_p and lib.dosx_wgrad_scratch_floats.restype is C.c_int64
    assert lib.dosx_version.restype is C.c_int and lib.dosx_version.argtypes == []


def test_abi_py_is_what_the_generator_makes_of_the_header(tmp_path):
    """dostransformer_amd/_abi.py is GENERATED (tools/gen_ctypes.py, run by csrc/Makefile): the committed file is the
    generator's output for the committed header, byte for byte."""
    gen = _gen("gen_ctypes")
    committed = open(os.path.join(ROOT, "dostransformer_amd", "_abi.py")).read()
    assert committed.startswith("# GENERATED by tools/gen_ctypes.py from include/dosx.h") and "do not edit" in committed.splitlines()[0]
    sys.argv, argv = ["gen", HEADER, str(tmp_path / "abi.py")], sys.argv
    try:
        gen.main()
    finally:
        sys.argv = argv
    assert (tmp_path / "abi.py").read_text() == committed
    assert gen.generate(open(HEADER).read()) == committed                       # deterministic


@pytest.mark.parametrize("line, what", [
    ("typedef struct DosxA { int32_t n; uint8_t x; } DosxA;", "uint8_t"),                 # unknown field type
    ("int dosx_f(const float* x, short n, dosx_stream_t stream);", "short"),            # unknown parameter type
    ("unsigned dosx_f(int n);", "unsigned"),                                            # unknown return type
    ("typedef struct DosxA { int32_t a[DOSX_N]; } DosxA;", "array size"),                # non-literal array size
    ("typedef struct DosxA { int32_t a : 3; } DosxA;", "a : 3"),                         # bit-field
    ("typedef struct DosxA { int32_t n; union { float f; int32_t i; } u; } DosxA;", "DosxA"),
    ("typedef struct DosxA { int (*fn)(int); } DosxA;", "fn"),                           # function pointer
    ("typedef struct DosxA { const float* p, q; } DosxA;", "one pointer"),               # `q` would not be a pointer
    ("typedef struct DosxA { DosxA* next; } DosxA;", "DosxA*"),                          # no pointer-to-struct fields
    ("enum { DOSX_X = 1 << 3 };", "DOSX_X"),                                            # not an integer literal
])
def test_generator_refuses_what_it_cannot_map(line, what):
    """A declaration outside the header's closed set of types stops the generator, with the header line in the message."""
    gen = _gen("gen_ctypes")
    header = "#include <stdint.h>\n/* a comment\n   of two lines */\ntypedef void* dosx_stream_t;\n" + line + "\nint dosx_version(void);\n"
    with pytest.raises(gen.Unmapped) as e:
        gen.generate(header)
    assert "dosx.h:5:" in str(e.value) and what in str(e.value) and line in str(e.value), str(e.value)
    assert "SIGS = {" in gen.generate(header.replace(line, "int dosx_g(int n);"))       # the frame around the line is fine


def test_python_constants_equal_the_header_enumerators():
    """No Python literal restates the header: every PRO_* / EPI_* / ACT64_* / ATTN* / COLSUM64_* name of ops.py, and every
    DOSX_* of _abi.py, has the value the header text gives its enumerator or #define."""
    from dostransformer_amd import _abi, ops
    from dostransformer_amd.layers import multihead_attention as mha
    header = _header_constants()
    assert len(header) >= 24 and header["DOSX_EPI_PRELU_LN_BWD_SEG"] == 7 and header["DOSX_OP_HIP_BASE"] == 1000
    assert {k: v for k, v in vars(_abi).items() if k.startswith("DOSX_")} == header
    named = [k for k in vars(ops) if re.match(r"(PRO|EPI|ACT64)_[A-Z]", k)]
    assert len(named) == 4 + 8 + 4 and all("DOSX_" + k in header for k in named), named
    shared = [k[5:] for k in header if hasattr(ops, k[5:])]
    assert set(named) | {"ATTN_RAW_Q", "ATTN_NO_RESIDUAL", "ATTN_BWD_DKV_HALF", "ATTN_BWD_DQ_HALF", "COLSUM64_ROWS", "ATTN64_MAX_H",
                         "ATTN64_SOFTMAX_F64"} == set(shared)
    for k in shared:
        assert getattr(ops, k) == header["DOSX_" + k], k
    assert (mha.RAW_Q, mha.NO_RESIDUAL) == (header["DOSX_ATTN_RAW_Q"], header["DOSX_ATTN_NO_RESIDUAL"])
    # DosxGemm.act has no enumerator; the header states its values in the comment of DOSX_EPI_BIAS_ACT
    act = re.search(r"act: (\d) none, (\d) relu, (\d) leaky\(slope\)", open(HEADER).read())
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY) == tuple(int(v) for v in act.groups())
    assert [k for k in vars(ops) if re.match(r"ACT_[A-Z]", k)] == ["ACT_NONE", "ACT_RELU", "ACT_LEAKY"]


def test_argument_validation_needs_no_gpu():
    """Entry points validate descriptors before touching the device and report through dosx_last_error."""
    from dostransformer_amd import _lib
    lib = _lib.load()
    g = _lib.Gemm()
    g.M, g.N, g.K, g.nseg = 4, 8, 0, 1
    assert lib.dosx_gemm(C.byref(g), None) != 0
    assert b"K=0" in lib.dosx_last_error()
    assert lib.dosx_gemm(None, None) != 0
    assert lib.dosx_wgrad_splits(9000, 256, 384) >= 1
    # one partial row per workgroup: 16-row tiles for small grids, 48-row tiles for M = 9000 (gemm_rt in csrc/gemm.hip)
    assert lib.dosx_gemm_partial_rows(100, 256, 2) == 7 and lib.dosx_gemm_partial_rows(100, 256, 5) == 14
    assert lib.dosx_gemm_partial_rows(9000, 256, 2) == 188 and lib.dosx_gemm_partial_rows(13056, 128, 4) == 204
    assert lib.dosx_ffn_bwd_partial_rows(3264) == 204 and lib.dosx_ffn_bwd_partial_rows(6528) == 204


def test_tail_entry_points_validate_before_any_launch():
    """The loss / AdamW / utility entry points refuse bad sizes, null pointers and misaligned buffers through DOSX_CHECK_ARG
    (rc -22 and a message naming the entry point), which stands in front of every launch; the pointers here are never
    dereferenced."""
    from dostransformer_amd import _lib
    lib = _lib.load()
    A, B, D, E = 0x10000, 0x20000, 0x30000, 0x40000          # 16-byte aligned fake device addresses

    def refused(rc, msg):
        assert rc == -22, rc
        assert msg in lib.dosx_last_error(), lib.dosx_last_error()

    adam = lambda p, g, m, v, n, step: lib.dosx_adamw(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, 1.0, None)
    assert adam(A, B, D, E, 0, 1) == 0 and adam(None, None, None, None, 0, 0) == 0     # n = 0: nothing to do
    refused(adam(A, B, D, E, 8, 0), b"dosx_adamw: bad args")
    refused(adam(A, B, D, E, 8, -3), b"dosx_adamw: bad args")
    refused(adam(None, B, D, E, 8, 1), b"dosx_adamw: bad args")
    for bad in range(4):
        ptrs = [A, B, D, E]
        ptrs[bad] += 4
        refused(adam(*ptrs, 8, 1), b"dosx_adamw: buffers must be 16-byte aligned")
    refused(lib.dosx_sse2(A, B, D, E, 0, None), b"dosx_sse2: bad args")
    refused(lib.dosx_sse2(A, B, D, E, -5, None), b"dosx_sse2: bad args")
    refused(lib.dosx_sse2(A, B, D, None, 51, None), b"dosx_sse2: bad args")
    refused(lib.dosx_sse2(None, B, D, E, 51, None), b"dosx_sse2: bad args")
    refused(lib.dosx_loss_phonon(A, B, D, None, 0.7, E, E, None, 0, None), b"dosx_loss_phonon: bad args")
    refused(lib.dosx_loss_phonon(A, B, None, None, 0.7, E, E, None, 51, None), b"dosx_loss_phonon: bad args")
    refused(lib.dosx_loss_phonon(A, B, D, None, 0.7, None, E, None, 51, None), b"dosx_loss_phonon: bad args")
    refused(lib.dosx_loss_phonon_bwd(A, B, D, E, 0.7, 51.0, E, E, None, 0, None), b"dosx_loss_phonon_bwd: bad args")
    refused(lib.dosx_loss_phonon_bwd(A, B, D, E, 0.7, 0.0, E, E, None, 51, None), b"dosx_loss_phonon_bwd: bad args")
    refused(lib.dosx_loss_phonon_bwd(A, B, D, None, 0.7, 51.0, E, E, None, 51, None), b"dosx_loss_phonon_bwd: bad args")
    refused(lib.dosx_loss_edos(A, B, D, 0.5, 0, 201, 4, E, E, E, None), b"dosx_loss_edos: bad args")
    refused(lib.dosx_loss_edos(A, B, D, 0.5, 4, 0, 4, E, E, E, None), b"dosx_loss_edos: bad args")
    refused(lib.dosx_loss_edos(A, B, D, 0.5, 4, 201, 0, E, E, E, None), b"dosx_loss_edos: bad args")
    refused(lib.dosx_loss_edos(A, B, D, 0.5, 4, 201, -1, E, E, E, None), b"dosx_loss_edos: bad args")
    refused(lib.dosx_loss_edos(A, B, D, 0.5, 4, 201, 4, E, E, None, None), b"dosx_loss_edos: bad args")
    refused(lib.dosx_sum(A, 0, B, None), b"dosx_sum: bad args")
    refused(lib.dosx_sum(None, 7, B, None), b"dosx_sum: bad args")
    refused(lib.dosx_sum(A, 7, None, None), b"dosx_sum: bad args")
    assert lib.dosx_act_bwd(A, B, 0.01, D, 0, None) == 0
    for n in (1, 6, 1023):
        refused(lib.dosx_act_bwd(A, B, 0.01, D, n, None), b"dosx_act_bwd: bad args (n must be a multiple of 4)")
    refused(lib.dosx_act_bwd(A, None, 0.01, D, 8, None), b"dosx_act_bwd: bad args")
    assert lib.dosx_reduce_rows(A, 32, B, 32, 0, 4, 4, 1, 32, 0, None) == 0
    refused(lib.dosx_reduce_rows(A, 32, B, 32, 5, 4, 4, 1, 30, 0, None), b"dosx_reduce_rows: bad args")       # width
    refused(lib.dosx_reduce_rows(A, 32, B, 32, 5, 4, 4, 1, 0, 0, None), b"dosx_reduce_rows: bad args")
    refused(lib.dosx_reduce_rows(A, 34, B, 32, 5, 4, 4, 1, 32, 0, None), b"dosx_reduce_rows: bad args")       # ld_src
    refused(lib.dosx_reduce_rows(A, 32, B, 33, 5, 4, 4, 1, 32, 0, None), b"dosx_reduce_rows: bad args")       # ld_dst
    refused(lib.dosx_reduce_rows(None, 32, B, 32, 5, 4, 4, 1, 32, 0, None), b"dosx_reduce_rows: bad args")


def test_product_path_fails_loudly_without_gpu():
    import torch
    from dostransformer_amd import synth
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.layers import TransformerEncoder
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    model = DOSTransformer_phonon(3, 1, 118, 4, 16, "cpu", 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(synth.phonon_batch(2, seed=0, dtype=torch.float32))
    enc = TransformerEncoder(16, 1, 1)
    x = torch.zeros(3, 2, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(x, x, x)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "dostransformer_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py") and f != "smoke.py":       # smoke.py is __graft_entry__.smoke()'s body (checker allowed)
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), (dp, f)


def test_replay_thunks_cover_the_header_and_are_typed():
    """dosx_replay dispatches through thunks GENERATED from include/dosx.h (tools/gen_replay_thunks.py): every `int
    dosx_*` entry point that fits a DosxCall has an op, with the argument-class counts of its prototype; the committed
    replay_thunks.inc is what the generator produces from the committed header."""
    from dostransformer_amd import _lib
    lib = _lib.load()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_replay_thunks as gen
    protos = list(gen.prototypes(open(HEADER).read()))
    assert len(protos) >= 40
    seen = set()
    for name, params in protos:
        ni = sum(1 for t in params if t not in gen.FLOAT_TYPES)
        nf = len(params) - ni
        a, b = C.c_int(-1), C.c_int(-1)
        op = lib.dosx_replay_op(name.encode(), C.byref(a), C.byref(b))
        if ni > 19 or nf > 6:
            assert op == -1, name                       # does not fit a DosxCall: not replayable
            continue
        assert op >= 0 and (a.value, b.value) == (ni, nf), (name, op, a.value, b.value, ni, nf)
        assert op not in seen
        seen.add(op)
    for name, n in (("hipEventRecord", 2), ("hipStreamWaitEvent", 3)):
        a = C.c_int(-1)
        assert lib.dosx_replay_op(name.encode(), C.byref(a), None) >= 1000 and a.value == n
    assert lib.dosx_replay_op(b"no_such_entry", None, None) == -1
    # a call whose argument counts do not match its entry point is rejected before anything is launched
    c = _lib.Call()
    c.op, c.nint, c.nflt = lib.dosx_replay_op(b"dosx_fill", None, None), 2, 1
    failed = C.c_int(-1)
    assert lib.dosx_replay((_lib.Call * 1)(c), 1, C.byref(failed)) != 0 and failed.value == 0
    assert b"dosx_fill" in lib.dosx_last_error()
    out = os.path.join(ROOT, "dostransformer_amd", "csrc", "replay_thunks.inc")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        sys.argv, argv = ["gen", HEADER, os.path.join(d, "t.inc")], sys.argv
        try:
            gen.main()
        finally:
            sys.argv = argv
        assert open(os.path.join(d, "t.inc")).read() == open(out).read()


def test_gemm_kernel_name_matches_the_tile_choice():
    from dostransformer_amd import _lib
    lib = _lib.load()
    g = _lib.Gemm()
    g.M, g.N, g.K, g.nseg = 9000, 256, 384, 1
    g.w_layout, g.pro, g.epi = 0, 0, 1
    g.a[0].ld, g.a[0].width = 384, 384
    g.ldw = 384
    buf = C.create_string_buffer(96)
    assert lib.dosx_gemm_kernel_name(C.byref(g), buf, 96) == 0
    assert buf.value == b"gemm_kernel<3, 2, 0, 0, 1, 1>"       # 48-row tiles, 256 columns, LN epilogue (edge GEMM1 at cfg2)


# ---- the host policies of the library, pinned ----------------------------------------------------------------------------
_POLICY_M = (1, 16, 17, 32, 33, 100, 3264, 4096, 4097, 6528, 8192, 8193, 9000, 12288, 12289, 12864, 13056, 16383, 16384, 17880,
             24576, 25728, 32769, 262144)
_POLICY_NK = (64, 128, 256, 384, 512, 1024)
# (label, M, N, K, w_layout, pro, epi, lda, fake stats_out / norm_out address): what dosx_gemm_kernel_name is asked for
_POLICY_GEMMS = (
    ("edge_gemm1_ln", 9000, 256, 384, 0, "NONE", "LN", 384, None),               # test_gemm_kernel_name_matches_the_tile_choice
    ("tail_split_relu_mask", 25728, 128, 512, 1, "NONE", "RELU_MASK", 512, None),
    ("ln_512_columns", 17880, 512, 256, 0, "NONE", "LN", 256, None),
    ("prelu_ln_bwd_512_columns", 17880, 512, 256, 1, "NONE", "PRELU_LN_BWD", 256, None),
    ("unaligned_atom_features", 1554, 128, 118, 0, "NONE", "BIAS_ACT", 118, None),
    ("one_half_tile", 16, 128, 128, 0, "NONE", "BIAS_ACT", 128, None),
    ("small_grid", 100, 256, 256, 0, "NONE", "BIAS_ACT", 256, None),
    ("fc1_forward", 12864, 512, 128, 0, "NONE", "BIAS_ACT", 128, None),
    ("fc1_forward_rowln", 25728, 512, 128, 0, "ROWLN", "BIAS_ACT", 128, None),
    ("rowln_bwd_256_columns", 25728, 256, 512, 1, "NONE", "ROWLN_BWD", 512, None),
    ("prelu_ln_bwd", 9000, 256, 256, 1, "NONE", "PRELU_LN_BWD", 256, None),
    ("prelu_bwd", 9000, 128, 128, 1, "NONE", "PRELU_BWD", 128, None),
    ("stats_out_256_columns", 6528, 256, 128, 0, "NONE", "BIAS_ACT", 128, "stats_out"),
    ("norm_out_512_columns", 6528, 512, 128, 0, "NONE", "BIAS_ACT", 128, "norm_out"),
    ("segsum", 4000, 128, 256, 0, "LN_PRELU", "SEGSUM", 256, None),
)


def _host_policy_table(lib):
    """Every exported host decision of csrc/gemm.hip and csrc/ffn.hip over a grid that straddles each threshold the policies
    contain, as JSON-ready lists in the order of the loops below."""
    from dostransformer_amd import _abi, _lib
    epis = sorted(v for k, v in vars(_abi).items() if k.startswith("DOSX_EPI_"))
    assert epis == list(range(8))
    t = {}
    t["gemm_partial_rows"] = [lib.dosx_gemm_partial_rows(M, N, e) for M in _POLICY_M for N in (64, 128, 256, 512) for e in epis]
    t["wgrad_splits"] = [lib.dosx_wgrad_splits(M, N, K) for M in _POLICY_M for N in _POLICY_NK for K in _POLICY_NK]
    t["wgrad_scratch_floats"] = [lib.dosx_wgrad_scratch_floats(N, K, s) for N in _POLICY_NK for K in _POLICY_NK for s in (1, 2, 8, 64)]
    t["ffn_bwd_partial_rows"] = [lib.dosx_ffn_bwd_partial_rows(M) for M in _POLICY_M]
    shapes = ((51, 64), (51, 1), (128, 64), (200, 8), (64, 64), (65, 64), (32, 128), (32, 129))    # 128 workgroups of 32 rows and one more
    t["ffn_att_bwd_partial_rows"] = [lib.dosx_ffn_att_bwd_partial_rows(Sq, Bq) for Sq, Bq in shapes]
    t["ffn_att_aligned_rows"] = [lib.dosx_ffn_att_aligned_rows(Sq, Bq) for Sq, Bq in shapes]
    hs, nks = (32, 64, 96, 128, 160), (1, 16, 17, 48, 64, 65)
    t["ffn_att_aligned_supported"] = [lib.dosx_ffn_att_aligned_supported(H, Nk) for H in hs for Nk in nks]
    t["ffn_att_bwd_supported"] = [lib.dosx_ffn_att_bwd_supported(H, Nk, Sq, Bq) for H in hs for Nk in nks for Sq, Bq in shapes[:4]]
    names = {}
    for label, M, N, K, wl, pro, epi, lda, extra in _POLICY_GEMMS:
        g = _lib.Gemm()
        g.M, g.N, g.K, g.nseg, g.w_layout = M, N, K, 1, wl
        g.pro, g.epi = getattr(_abi, "DOSX_PRO_" + pro), getattr(_abi, "DOSX_EPI_" + epi)
        g.a[0].ld, g.a[0].width, g.ldw = lda, K, (K if wl == 0 else N)
        if extra:
            setattr(g, extra, 0x10000)                   # (an address that is only tested against NULL)
        buf = C.create_string_buffer(96)
        assert lib.dosx_gemm_kernel_name(C.byref(g), buf, 96) == 0
        names[label] = buf.value.decode()
    t["gemm_kernel_name"] = names
    return t


def test_host_policies_are_those_of_the_commit_that_folded_their_switches():
    """tests/golden/host_policy.json was recorded from a library built at the commit BEFORE the getenv tuning switches of
    csrc/ were folded into constants, with no DOSX_* variable set
    (DOSX_LIB=<that build> python -c "import json; from tests.test_lib_abi import _host_policy_table as t; from
    dostransformer_amd import _lib; print(json.dumps(t(_lib.load())))"): tile heights, column tiles, tail splits, weight-gradient
    splits and scratch sizes, the feed-forward half-tile threshold and chunk width are what they were, value for value."""
    import json
    from tests.util import GOLDEN, dosx_lib
    want = json.load(open(os.path.join(GOLDEN, "host_policy.json")))
    got = _host_policy_table(dosx_lib().load())
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    assert len(want["gemm_partial_rows"]) == 24 * 4 * 8 and len(want["wgrad_splits"]) == 24 * 36 and len(want["gemm_kernel_name"]) >= 12
    # the table is not degenerate: every tile height and the tail split occur
    assert want["gemm_kernel_name"]["edge_gemm1_ln"] == "gemm_kernel<3, 2, 0, 0, 1, 1>"
    assert want["gemm_kernel_name"]["unaligned_atom_features"].endswith("0, 0, 0>")
    assert {n.split("<")[1][0] for n in want["gemm_kernel_name"].values()} == set("0123")
    assert set(want["wgrad_splits"]) >= {1, 8, 64} and set(want["ffn_att_aligned_rows"]) == {16, 32}


def test_gemm_census_is_complete():
    """tests/gemm_census.py lists every instantiation of gemm_kernel / gemm_mixed_kernel / gemm_pair_kernel a valid descriptor
    reaches.  (1) dosx_gemm_kernel_name over the policy grid of M, tile-straddling N, every family, stats_out / norm_out set and
    clear names nothing without a census row; (2) every row's shapes still select the kernel the row names, leave one row / all
    but one row in the last tile, and are the smallest that do; a tail split shows in dosx_gemm_partial_rows exactly where the
    census says; (3) what the census lists as refused is refused, before any launch.  A new instantiation or a moved policy
    threshold fails here, on the CPU."""
    from dostransformer_amd import _abi, _lib
    from tests import gemm_census as cen
    lib = _lib.load()
    name = lambda M, N, fam, pro, epi, extra="", K=64: cen.kernel_name(lib, cen.fake_desc(M, N, K, fam, pro, epi, extra))
    known = {}
    for fam, pro, epi, extra, kernel, *_ in cen.ROWS + cen.REFUSED:
        known.setdefault((fam, pro, epi), set()).add(kernel)
    for fam, pro, epi, kernel, *_ in cen.SEG_ROWS:
        known.setdefault((fam, pro, epi), set()).add(kernel)
    assert len({k for v in known.values() for k in v}) == len(cen.ROWS) + len(cen.SEG_ROWS) + len(cen.REFUSED)   # no kernel twice
    assert cen.n_instantiations() == 117
    # (1) the sweep.  Left out: what gemm_validate refuses by shape alone (a full-row epilogue, stats_out or norm_out beyond 512
    # columns, node-aligned tiles beyond 256) and norm_out behind another epilogue than the plain one
    full_row = ("LN", "PRELU_LN_BWD", "ROWLN_BWD", "PRELU_LN_BWD_SEG")
    swept = set()
    for fam, (wl, vec, pros, epis) in cen.FAMILIES.items():
        for pro in pros:
            for epi in epis:
                for extra in ("", "stats", "norm"):
                    if extra == "norm" and epi != "BIAS_ACT":
                        continue
                    for N in cen.SWEEP_N:
                        if N > 512 and (extra or epi in full_row) or N > 256 and epi in ("SEGSUM", "PRELU_LN_BWD_SEG"):
                            continue
                        for M in _POLICY_M:
                            k = name(M, N, fam, pro, epi, extra)
                            assert k in known[(fam, pro, epi)], (k, fam, pro, epi, extra, M, N)
                            swept.add(k)
    assert len(swept) == len(cen.ROWS) + len(cen.SEG_ROWS) + len(cen.REFUSED)              # and the grid reaches every row
    # (2) the rows
    for fam, pro, epi, extra, kernel, *shapes in cen.ROWS:
        h = cen.tile_rows(kernel)
        for N, m_one, m_short in shapes:
            assert m_one % h == 1 and m_short % h == h - 1 and min(m_one, m_short) > h, (kernel, N)
            for M in (m_one, m_short):
                assert name(M, N, fam, pro, epi, extra) == kernel, (kernel, M, N)
                assert extra or not cen.is_split(lib, M, N, epi, kernel), (kernel, M, N)
            assert m_one - h <= h or name(m_one - h, N, fam, pro, epi, extra) != kernel, (kernel, N, "not the smallest")
    for fam, pro, epi, kernel, n_full, n_rag in cen.SEG_ROWS:
        assert {name(M, N, fam, pro, epi) for M in (1, 700, 20000) for N in (n_full, n_rag)} == {kernel}
    for fam, pro, epi, mixed, head, *shapes in cen.MIXED_ROWS:
        ha, hb = (cen.TILE_ROWS[int(v)] for v in re.match(r"gemm_mixed_kernel<(\d), (\d)", mixed).groups())
        assert ha == cen.tile_rows(head) and mixed.split(", ", 2)[2] == head.split(", ", 1)[1]      # same NTW, WL, PRO, VEC, EPI
        for N, m_one, m_short, p_one, p_short in shapes:
            for M, p in ((m_one, p_one), (m_short, p_short)):
                assert name(M, N, fam, pro, epi) == head and cen.is_split(lib, M, N, epi, head), (mixed, M, N)
                assert lib.dosx_gemm_partial_rows(M, N, getattr(_abi, "DOSX_EPI_" + epi)) == p, (mixed, M, N)
                tiles = -(-N // (128 * int(head.split(", ")[1])))                     # column tiles: 256 / tiles head tiles a round
                full = M // (256 // tiles * ha) * (256 // tiles * ha)
                assert p == full // ha + -(-(M - full) // hb) and (M - full) % hb in (1, hb - 1), (mixed, M, N)
    for kernel, head, extra, n_full, n_rag, m1, m2 in cen.PAIR_ROWS:
        rt, ntw = re.match(r"gemm_pair_kernel<(\d), (\d)>", kernel).groups()
        assert head == f"gemm_kernel<{rt}, {ntw}, 0, 0, 1, 0>"
        for N in (n_full, n_rag):
            assert name(m1 + m2, N, "plain_nk", "NONE", "BIAS_ACT", extra) == head, (kernel, N)
            for M in (m1, m2):                                       # (each problem alone plans the same column tile)
                assert name(M, N, "plain_nk", "NONE", "BIAS_ACT", extra).split(", ")[1] == ntw, (kernel, M, N)
    kernel, head_a, head_b, N, m1, m2 = cen.PAIR_MIXED
    assert name(m1, N, "bwd", "NONE", "PRELU_BWD") == head_a and name(m2, N, "bwd", "NONE", "PRELU_BWD") == head_b
    assert not cen.is_split(lib, m1, N, "PRELU_BWD", head_a) and not cen.is_split(lib, m2, N, "PRELU_BWD", head_b)
    # (3) refused before any launch (the addresses are never dereferenced)
    ident = _lib.RowMap(1 << 30, 0, 1, 0, None)

    def refused(g, msg):
        g.a[0].p, g.a[0].map, g.w, g.out, g.ldo, g.out_map = 0x10000, ident, 0x20000, 0x30000, g.N, ident
        g.pro_gamma = g.pro_beta = g.pro_alpha = g.pro_stats = g.aux = g.epi_alpha = 0x40000
        g.ldaux = g.N
        assert lib.dosx_gemm(C.byref(g), None) == -22 and msg.encode() in lib.dosx_last_error(), (msg, lib.dosx_last_error())

    for fam, pro, epi, extra, kernel, M, N, msg in cen.REFUSED:
        assert name(M, N, fam, pro, epi, extra) == kernel
        refused(cen.fake_desc(M, N, 64, fam, pro, epi, extra), msg)
    # no descriptor reaches the generic staging path with N % 4 != 0: the output rows are stored as float4
    refused(cen.fake_desc(100, 130, 41, "generic_nk", "NONE", "BIAS_ACT"), "4-float aligned")
