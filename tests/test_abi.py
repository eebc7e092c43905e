"""CPU: the C-ABI library builds, loads without a GPU, and exports every symbol that
include/cloops_hip.h declares; no compute is attempted.  The ctypes side -- the binding tables of _lib and comm, the structs and the
restated constants -- agrees with the headers, prototype by prototype."""
import ctypes
import os
import re

import numpy as np
import pytest

from cloops_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    with open(os.path.join(ROOT, "include", "cloops_hip.h")) as fh:
        src = fh.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cl_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported():
    so = build.build()
    lib = ctypes.CDLL(so)
    names = declared_symbols()
    assert len(names) >= 12
    for n in names:
        assert getattr(lib, n) is not None, n
    assert sorted(_lib.SYMBOLS) == names


def test_version_and_error_plumbing_without_gpu():
    lib = _lib.load()
    assert lib.cl_version() >= 100
    if lib.cl_device_count() == 0:
        # no CPU fallback: creating a chromosome must fail loudly
        from cloops_amd import api
        with pytest.raises(_lib.CloopsHipError) as ei:
            api.Chromosome(np.arange(4), np.arange(4) + 5)
        assert ei.value.code == _lib.CL_ERR_NODEVICE
        from cloops_amd.cDBSCAN2 import cDBSCAN
        with pytest.raises(_lib.CloopsHipError):
            cDBSCAN(np.array([[0, 1, 2], [1, 2, 3]]), 5, 2)


def test_missing_library_is_an_import_error(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", "/nonexistent/libcloops_hip.so")
    with pytest.raises(ImportError):
        _lib.load()


def test_header_is_plain_c(tmp_path):
    """include/cloops_hip.h is C (not C++): the plain-C consumer of tests/c compiles against it with -Werror"""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), "-c",
                           os.path.join(root, "tests", "c", "abi_smoke.c"), "-o", os.path.join(str(tmp_path), "a.o")])


# ---- the binding tables, the structs and the constants against the headers (no GPU, no built library) ----------------------------
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "char": ctypes.c_char}
STRUCTS = {"cl_box": _lib.ClBox, "cl_timing": _lib.ClTiming, "cl_dsummary": _lib.ClDsummary, "cl_ingest_name": _lib.ClIngestName}


def header_text(name):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def header_defines(src):
    """the #defines with an integer value -> {name: value}"""
    return {n: int(v) for n, v in re.findall(r"^\s*#define\s+(CL_\w+)\s+(-?\d+)\s*$", src, flags=re.M)}


def c_type(text):
    """a C type as written -> its name without qualifiers and blanks, one '*' per level: 'const int32_t* const*' -> 'int32_t**'"""
    return re.sub(r"\bconst\b|\s+", "", text)


def header_prototypes(src):
    """every `ret cl_name(params);` of a header -> {name: (return type, [parameter types])}"""
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(cl_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
        assert name not in out, name
        params = [p.strip() for p in params.split(",")]
        if params == ["void"]:
            params = []
        types = []
        for p in params:
            m = re.match(r"^(.*?)\b[A-Za-z_]\w*$", p, flags=re.S)          # the type is what stands before the parameter's name
            assert m and m.group(1).strip(), "%s: parameter %r" % (name, p)
            types.append(c_type(m.group(1)))
        out[name] = (c_type(ret), types)
    return out


def header_structs(src, defines):
    """every `typedef struct [tag] { fields } name;` -> {name: [(field, scalar C type, array length or None)]}"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            typ, names = decl.split(None, 1)
            for f in names.split(","):
                m = re.match(r"^(\w+)(?:\[(\w+)\])?$", f.strip())
                assert m, "%s: field %r" % (name, f)
                n = m.group(2)
                fields.append((m.group(1), typ, None if n is None else int(n) if n.isdigit() else defines[n]))
        out[name] = fields
    return out


def kinds_of(ctype):
    """the ctypes types that may stand for the C type `ctype` in a binding table"""
    if ctype == "void":
        return [None]
    if not ctype.endswith("*"):
        return [SCALARS[ctype]]
    target = ctype[:-1]
    ok = [ctypes.c_void_p]
    if target == "char":
        ok.append(ctypes.c_char_p)
    if target.endswith("*"):
        ok.append(ctypes.POINTER(ctypes.c_void_p))                         # a pointer to any pointer
    elif target in SCALARS:
        ok.append(ctypes.POINTER(SCALARS[target]))
    elif target in STRUCTS:
        ok.append(ctypes.POINTER(STRUCTS[target]))
    return ok                                                              # (void* and pointers to opaque handles: c_void_p only)


def table_faults(table, protos):
    """-> what differs between a binding table and the prototypes of its header, one line each"""
    faults = []
    if set(table) != set(protos):
        faults.append("names differ: %s" % sorted(set(table) ^ set(protos)))
    for name, (ret, params) in sorted(protos.items()):
        entry = table.get(name)
        if not (isinstance(entry, (tuple, list)) and len(entry) == 2 and isinstance(entry[1], (tuple, list))):
            faults.append("%s: needs (restype, [argtypes]), has %r" % (name, entry))
            continue
        restype, argtypes = entry
        want = [ctypes.c_char_p] if ret == "char*" else kinds_of(ret)      # a returned string comes back as bytes
        if not any(restype is w for w in want):
            faults.append("%s: returns %s, bound as %r" % (name, ret, restype))
        if len(argtypes) != len(params):
            faults.append("%s: %d parameters, %d argtypes" % (name, len(params), len(argtypes)))
            continue
        for k, (p, a) in enumerate(zip(params, argtypes)):
            if not any(a is w for w in kinds_of(p)):
                faults.append("%s: parameter %d is %s, bound as %r" % (name, k, p, a))
    return faults


def test_binding_table_matches_header():
    src = header_text("cloops_hip.h")
    protos = header_prototypes(src)
    assert sorted(protos) == declared_symbols()                            # the parser missed no declaration
    assert table_faults(_lib.PROTOTYPES, protos) == []
    assert _lib.SYMBOLS == list(_lib.PROTOTYPES)


def test_comm_binding_table_matches_header():
    from cloops_amd import comm
    src = header_text("cloops_comm.h")
    protos = header_prototypes(src)
    assert sorted(protos) == sorted(set(re.findall(r"\b(cl_comm_[a-z0-9_]+)\s*\(", src)))
    assert table_faults(comm.PROTOTYPES, protos) == []
    assert comm.SYMBOLS == tuple(comm.PROTOTYPES)
    assert header_defines(src) == {"CL_COMM_ID_BYTES": comm.ID_BYTES}


def test_the_table_check_bites():
    """a wrong width, a missing argument and a missing part are each reported (on copies: the tables themselves are right)"""
    protos = header_prototypes(header_text("cloops_hip.h"))
    i32p = ctypes.POINTER(ctypes.c_int32)
    ret, args = _lib.PROTOTYPES["cl_cand_append"]                           # (cl_chrom*, int32_t, int64_t*, int64_t*)
    for bad in ((ret, args[:2] + [i32p] + args[3:]), (ret, args[:-1]), (ret,), (ret, None), (ctypes.c_int64, args), (None, args),
                (ret, [ctypes.c_int64] + args[1:]), (ret, args[:1] + [ctypes.c_int64] + args[2:])):
        faults = table_faults(dict(_lib.PROTOTYPES, cl_cand_append=bad), protos)
        assert len(faults) == 1 and faults[0].startswith("cl_cand_append:"), (bad, faults)
    missing = {k: v for k, v in _lib.PROTOTYPES.items() if k != "cl_wait"}
    assert table_faults(missing, protos) != []
    assert table_faults(dict(_lib.PROTOTYPES, cl_last_error=(ctypes.c_void_p, [])), protos) != []


def test_structs_match_header():
    src = header_text("cloops_hip.h")
    structs = header_structs(src, header_defines(src))
    assert sorted(structs) == sorted(STRUCTS)
    for name, cls in STRUCTS.items():
        want = [(f, SCALARS[t] if n is None else SCALARS[t] * n) for f, t, n in structs[name]]
        got = list(cls._fields_)
        assert [f for f, _ in got] == [f for f, _ in want], name
        for (f, g), (_, w) in zip(got, want):
            if hasattr(w, "_length_"):
                assert hasattr(g, "_length_") and (g._type_, g._length_) == (w._type_, w._length_), "%s.%s" % (name, f)
            else:
                assert g is w, "%s.%s" % (name, f)
    from cloops_amd import api
    box = api.BOX_DTYPE
    assert box.itemsize == ctypes.sizeof(_lib.ClBox) and list(box.names) == [f for f, _ in _lib.ClBox._fields_]
    for f, t in _lib.ClBox._fields_:
        assert box.fields[f][0] == np.dtype(t) and box.fields[f][1] == getattr(_lib.ClBox, f).offset, f


def test_constants_match_header():
    """every integer #define of the header has ONE twin in _lib (CL_VARIANT_X is VARIANT_X there, CL_DIST_LOGBINS DIST_LOGBINS),
    and what api restates reads those"""
    from cloops_amd import api
    defines = header_defines(header_text("cloops_hip.h"))
    named = ["CL_OK", "CL_ERR_ARG", "CL_ERR_HIP", "CL_ERR_EMPTY", "CL_ERR_DOMAIN", "CL_ERR_GRID", "CL_ERR_NODEVICE", "CL_ERR_HASH", "CL_ERR_PARSE",
             "CL_VARIANT_CDBSCAN1", "CL_VARIANT_CDBSCAN2", "CL_VARIANT_BLOCK", "CL_DIST_LOGBINS", "CL_TRACK_WASHU", "CL_TRACK_JUICE",
             "CL_TRACK_NAME_MAX", "CL_CONV_HICPRO", "CL_CONV_JUICER", "CL_CONV_E_FIELDS", "CL_CONV_E_INT", "CL_CONV_E_RANGE", "CL_CONV_E_LONG",
             "CL_INGEST_TIMES"]
    assert set(named) <= set(defines)                                       # the parser missed none of the known ones
    for name, value in defines.items():
        twin = name[3:] if name.startswith("CL_VARIANT_") or name == "CL_DIST_LOGBINS" else name
        assert getattr(_lib, twin, None) == value, name
    assert api.Chromosome.TRACK_KINDS == {"washu": defines["CL_TRACK_WASHU"], "juice": defines["CL_TRACK_JUICE"]}
    assert api.Chromosome.TRACK_NAME_MAX == defines["CL_TRACK_NAME_MAX"]
    assert api.Converter.FORMATS == {"hicpro": defines["CL_CONV_HICPRO"], "juicer": defines["CL_CONV_JUICER"]}
    assert sorted(api.Converter.KINDS) == sorted(v for k, v in defines.items() if k.startswith("CL_CONV_E_"))
    assert len(api.Ingest.TIMES) == defines["CL_INGEST_TIMES"]
    assert {api.VARIANTS[k] for k in ("v1", "v2", "block")} == {v for k, v in defines.items() if k.startswith("CL_VARIANT_")}
