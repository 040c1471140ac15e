"""The ctypes table against the header, type by type: every prototype of include/audio_metrics_hip.h is parsed (no compiler)
and its return and argument types must be the ones _lib.SIGNATURES declares for that name.  test_abi_cpu.py compares the
names; an argument slipped by one position, or an int where the header says int64_t, shows up here."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
           "unsigned": ctypes.c_uint, "uint64_t": ctypes.c_uint64}
PROTOTYPE = re.compile(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(am_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.M)


def _ctype(decl, returned=False):
    """The ctypes type of a C declaration such as `const float* X`, `int64_t N`, `am_stream_t stream` or a bare return type."""
    decl = " ".join(decl.replace("*", " * ").split())
    if re.fullmatch(r"const char \*", decl) and returned:
        return ctypes.c_char_p
    words = [w for w in decl.split() if w != "const"]
    if "*" in words or words[0] == "am_stream_t":
        return ctypes.c_void_p
    assert words[0] in SCALARS, f"a type this test does not know: {decl!r}"
    assert len(words) == (1 if returned else 2), f"not `type name`: {decl!r}"
    return SCALARS[words[0]]


def header_prototypes():
    """name -> (restype, argtypes) of every function the header declares."""
    src = open(os.path.join(ROOT, "include", "audio_metrics_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for ret, name, args in PROTOTYPE.findall(src):
        assert name not in out, f"{name} is declared twice"
        args = " ".join(args.split())
        out[name] = (_ctype(ret, returned=True), [] if args in ("", "void") else [_ctype(a) for a in args.split(",")])
    return out


def test_signature_table_matches_the_header_type_by_type():
    import audio_metrics_amd as am
    table = am._lib.SIGNATURES
    protos = header_prototypes()
    assert len(protos) == len(table) and sorted(protos) == sorted(table)
    for name, (res, args) in protos.items():
        want_res, want_args = table[name]
        assert res is want_res, f"{name}: the header returns {res.__name__}, the table says {want_res.__name__}"
        assert len(args) == len(want_args), f"{name}: {len(args)} arguments in the header, {len(want_args)} in the table"
        for i, (a, b) in enumerate(zip(args, want_args)):
            assert a is b, f"{name}: argument {i} is {a.__name__} in the header, {b.__name__} in the table"
