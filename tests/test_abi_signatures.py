"""The headers judge the ctypes table: every prototype of the seven headers under include/ against
ms_amd/_lib.py SIGNATURES / _RESTYPES (parameter count, every scalar type, the pointee of every
typed pointer, the return type), the struct mirrors field by field, and the Python copies of the
headers' #define constants. CPU only; the built libraries are needed for the export checks alone."""
from __future__ import annotations

import ctypes
import glob
import os
import re

from conftest import PKG_DIR, ROOT
from test_abi import header_functions

HEADERS = [os.path.join(ROOT, "include", h) for h in
           ("msenv.h", "msenv_debug.h", "mscnn.h", "msppo.h", "mssolve.h", "msposterior.h", "msposterior_labels.h")]
# ctypes.c_int32 is the class ctypes.c_int where int has 32 bits (every platform the library builds
# for), so `int` and `int32_t` are not told apart: the check is exact in width and signedness
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
# what a POINTER(T) may point at, besides the struct mirrors
POINTEES = dict(SCALARS, int8_t=ctypes.c_int8, uint8_t=ctypes.c_uint8, uint16_t=ctypes.c_uint16,
                **{"unsigned long long": ctypes.c_ulonglong})
RETURNS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p,
           "void": None}
DECL = re.compile(r"^(?P<type>.+?[\s*])(?P<names>\w+(?:\s*,\s*\w+)*)$", re.S)  # `float a, b, c` too
PROTO = re.compile(r"^(?P<ret>[\w\s*]+?[\s*])(?P<name>\w+)\s*\((?P<params>[^()]*)\)$", re.S)


def _ctype(t: str, keep_const: bool = False) -> str:
    """`const  float *` -> `float*`."""
    if not keep_const:
        t = re.sub(r"\bconst\b", " ", t)
    return re.sub(r"\s*\*", "*", " ".join(t.split()))


def _decls(text: str, sep: str):
    """[(c type, name)] of a parameter list (sep ",") or a struct body (sep ";")."""
    out = []
    for d in (d.strip() for d in text.split(sep)):
        if d and d != "void":
            m = DECL.match(d)
            assert m, f"cannot parse declaration {d!r}"
            out += [(_ctype(m["type"]), n.strip()) for n in m["names"].split(",")]
    return out


def parse_headers(headers=HEADERS):
    """-> (protos {name: (return type, [(type, param)])}, structs {name: [(type, field)]},
    defines {name: int}, diag_only {names declared under #ifdef MC_DIAG}). Every statement that is
    left after comments, preprocessor lines, enums and struct bodies are taken out must parse as a
    prototype: nothing is skipped."""
    protos, structs, defines, diag_only = {}, {}, {}, set()
    for path in headers:
        src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path).read(), flags=re.S)
        for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(M[SC]_\w+|MSENV_ABI_VERSION)[ \t]+(.+?)[ \t]*$", src,
                                    flags=re.M):
            if re.fullmatch(r"[\s0-9a-fA-FxXuUlL()<>|&+*~-]+", val):
                defines[name] = eval(re.sub(r"(?<=[0-9a-fA-F])[uUlL]+\b", "", val), {"__builtins__": {}})
        for block in re.findall(r"^[ \t]*#[ \t]*ifdef[ \t]+MC_DIAG\b(.*?)^[ \t]*#[ \t]*endif", src, flags=re.S | re.M):
            diag_only |= set(re.findall(r"\b(m[sc]_\w+)\s*\(", block))
        src = re.sub(r"^[ \t]*#.*$", "", src, flags=re.M).replace('extern "C" {', "")
        for tag, body, name in re.findall(r"typedef\s+struct\s*(\w*)\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
            structs[name] = _decls(body, ";")
        src = re.sub(r"typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;|enum\s*\{.*?\}\s*;|typedef[^;{]*;", "", src, flags=re.S)
        src = src.replace("}", "", 1)  # the closing brace of extern "C"
        assert "{" not in src and "}" not in src, f"{path}: unparsed braces"
        for stmt in (s.strip() for s in src.split(";")):
            if stmt:
                m = PROTO.match(stmt)
                assert m, f"{path}: cannot parse {stmt!r}"
                assert m["name"] not in protos, f"{m['name']} is declared twice"
                protos[m["name"]] = (_ctype(m["ret"], keep_const=True), _decls(m["params"], ","))
    return protos, structs, defines, diag_only


def _mirrors():
    from ms_amd import _lib as L
    return {"ms_cfg": L.MsCfg, "mc_fwd_layer": L.McFwdLayer, "mc_bwd_layer": L.McBwdLayer,
            "mc_ppo_loss_args": L.McPpoLossArgs}


def _param_ok(ctype: str, argtype) -> bool:
    if ctype.endswith("**"):  # void**, ms_handle**: callers pass byref(c_void_p())
        return argtype is ctypes.POINTER(ctypes.c_void_p)
    if ctype.endswith("*"):
        pointee = _mirrors().get(ctype[:-1], POINTEES.get(ctype[:-1]))
        return argtype is ctypes.c_void_p or (pointee is not None and argtype is ctypes.POINTER(pointee))
    return ctype in SCALARS and argtype is SCALARS[ctype]


def table_errors(signatures, restypes, protos) -> list:
    """Every disagreement between the ctypes table and the parsed prototypes, one line each."""
    errs = [f"{name}: in SIGNATURES but in no header" for name in signatures if name not in protos]
    for name, (ret, params) in protos.items():
        if name not in signatures:
            errs.append(f"{name}: no ctypes signature")
            continue
        argtypes = signatures[name]
        if len(argtypes) != len(params):
            errs.append(f"{name}: {len(argtypes)} argtypes, the header has {len(params)} parameters")
            continue
        errs += [f"{name}: parameter {i} `{ct} {pn}` is bound as {at.__name__}"
                 for i, ((ct, pn), at) in enumerate(zip(params, argtypes)) if not _param_ok(ct, at)]
        restype = restypes.get(name, ctypes.c_int)  # load()'s default
        if ret not in RETURNS or restype is not RETURNS[ret]:
            errs.append(f"{name}: returns `{ret}`, restype is {getattr(restype, '__name__', restype)}")
    return errs


def test_parser_finds_every_declared_function():
    """Against a vacuous pass: the parser's names are exactly those the name-only regex finds."""
    protos, _, _, diag_only = parse_headers()
    names = set(header_functions(HEADERS, "ms_")) | set(header_functions(HEADERS, "mc_"))
    assert set(protos) == names
    assert len(names) >= 58
    assert diag_only <= names


def test_ctypes_table_matches_the_headers():
    from ms_amd import _lib as L
    protos, _, _, diag_only = parse_headers()
    assert table_errors(L.SIGNATURES, L._RESTYPES, protos) == []
    assert diag_only == L.DIAG_ONLY


def test_libraries_export_and_bind_every_function():
    """The product library exports every function but those under #ifdef MC_DIAG, which the
    diagnostic build exports; load() has put the table on every function it found. The product
    library is asked by symbol lookup (getattr). The diagnostic library is only read: its check is
    that the NUL-delimited name occurs in the file's bytes (its string tables), not a symbol lookup."""
    from ms_amd import _lib as L
    protos, _, _, diag_only = parse_headers()
    lib = L.load()
    with open(os.path.join(PKG_DIR, "libmsenv_diag.so"), "rb") as f:
        diag_image = f.read()  # read, not loaded: a second copy of the kernels stays out of the process
    for name in protos:
        assert b"\0" + name.encode() + b"\0" in diag_image, f"libmsenv_diag.so lacks {name}"
        if name in diag_only and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        assert list(fn.argtypes) == L.SIGNATURES[name], name
        assert fn.restype is L._RESTYPES.get(name, ctypes.c_int), name


def test_struct_mirrors_match_the_headers():
    _, structs, _, _ = parse_headers()
    mirrors = _mirrors()
    assert set(structs) == set(mirrors)
    for name, fields in structs.items():
        got = mirrors[name]._fields_
        assert [f for f, _ in got] == [f for _, f in fields], name
        for (ct, fname), (_, ft) in zip(fields, got):
            want = ctypes.c_void_p if ct.endswith("*") else SCALARS[ct]
            assert ft is want, f"{name}.{fname}: `{ct}` is mirrored as {ft.__name__}"
    args = mirrors["mc_ppo_loss_args"]  # 12 pointers, 2 int32, 8 floats, int64, int32
    assert ctypes.sizeof(args) == 152 and args.M.offset == 136 and args.A.offset == 144


def test_constants_match_the_headers():
    from ms_amd import _lib as L
    _, _, defines, _ = parse_headers()
    assert len(defines) >= 17
    checked = 0
    for name, val in defines.items():
        attr = "ABI_VERSION" if name == "MSENV_ABI_VERSION" else name
        if hasattr(L, attr):
            assert getattr(L, attr) == val, name
            checked += 1
    assert checked >= 17 and "MSENV_ABI_VERSION" in defines
    import torch
    from ms_amd import fused as F
    assert F.DTYPES == {torch.bfloat16: defines["MC_DTYPE_BF16"], torch.float16: defines["MC_DTYPE_F16"]}
    assert F.MAX_CHAIN_LAYERS == defines["MC_TRUNK_MAX_LAYERS"]
    assert (F.VARIANT_FWD, F.VARIANT_BWD, F.VARIANT_WGRAD, F.VARIANT_TRUNK_FWD) == tuple(
        defines[n] for n in ("MC_VAR_FWD", "MC_VAR_BWD", "MC_VAR_WGRAD", "MC_VAR_TRUNK_FWD"))


def test_checker_reports_a_wrong_table():
    from ms_amd import _lib as L
    protos = parse_headers()[0]

    def errors(name, argtypes=None, restype=None):
        sigs = {k: list(v) for k, v in L.SIGNATURES.items()}
        rets = dict(L._RESTYPES)
        if argtypes is not None:
            sigs[name] = argtypes
        if restype is not None:
            rets[name] = restype
        errs = table_errors(sigs, rets, protos)
        assert errs and all(e.startswith(name + ":") for e in errs), errs
        return errs

    narrowed = list(L.SIGNATURES["mc_heads_bwd"])
    narrowed[narrowed.index(ctypes.c_int64)] = ctypes.c_int32
    assert "int64_t" in errors("mc_heads_bwd", argtypes=narrowed)[0]
    assert "10 argtypes" in errors("ms_step", argtypes=L.SIGNATURES["ms_step"][:-1])[0]
    assert "int64_t" in errors("mc_trunk_bwd_workspace", restype=ctypes.c_int)[0]


def test_nothing_binds_outside_the_table():
    """No .argtypes / .restype assignment outside ms_amd/_lib.py (oracle/ binds another library)."""
    files = [os.path.join(ROOT, "train_rl.py")]
    for d in (os.path.join(PKG_DIR, "ms_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
        files += glob.glob(os.path.join(d, "**", "*.py"), recursive=True)
    own = (os.path.join(PKG_DIR, "ms_amd", "_lib.py"), os.path.abspath(__file__))
    hits = []
    for path in files:
        if os.path.abspath(path) in own:
            continue
        for i, line in enumerate(open(path), 1):
            if re.search(r"\.(argtypes|restype)\b[^=\n]*=(?!=)", line):
                hits.append(f"{os.path.relpath(path, ROOT)}:{i}: {line.strip()}")
    assert hits == []
