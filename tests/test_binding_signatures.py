"""The binding's signature table (bmx.SIGNATURES: name -> (restype, argtypes), applied by load_library()) held against the prototypes of include/*.h. No GPU
and no built library: the table is read as data. A uint32_t declared where the header has a uint64_t is undefined behaviour that the x86-64 calling convention
usually hides, so every parameter of every function is compared by class."""
import ctypes as C
import glob
import os
import re

import bmx

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"uint64_t": "u64", "uint32_t": "u32", "int64_t": "i64", "int": "int", "double": "double", "float": "float"}
CTYPES = {C.c_uint64: "u64", C.c_uint32: "u32", C.c_int64: "i64", C.c_int: "int", C.c_double: "double", C.c_float: "float", C.c_void_p: "ptr", C.c_char_p: "ptr", None: "void"}


def c_class(decl, what):
    """one C parameter or return type -> its class: any pointer or T name[N] is "ptr", a scalar is its type"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in re.findall(r"\w+", decl) if w != "const"]
    assert words and words[0] in SCALARS or words == ["void"], "%s: unknown C type in %r" % (what, decl)
    return "void" if words == ["void"] else SCALARS[words[0]]


def ctypes_class(t, what):
    if t not in CTYPES:
        assert isinstance(t, type) and issubclass(t, C._Pointer), "%s: unknown ctypes type %r" % (what, t)
        return "ptr"
    return CTYPES[t]


def prototypes():
    """-> {name: (return class, [parameter classes])} of every bmx_* function the headers declare"""
    out = {}
    for path in sorted(glob.glob(os.path.join(INCLUDE, "*.h"))):
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^\s*#[^\n]*(\\\n[^\n]*)*", " ", text, flags=re.M)          # preprocessor lines, continued ones included
        for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(bmx_\w+)\s*\(([^()]*)\)\s*;", text):
            assert name not in out, "%s is declared twice" % name
            params = [p.strip() for p in params.split(",")]
            if params in ([""], ["void"]):
                params = []
            out[name] = (c_class(ret, name), [c_class(p, name) for p in params])
    return out


def test_the_table_names_what_the_headers_declare():
    declared = prototypes()
    assert set(declared) == set(bmx.SIGNATURES)
    assert len(declared) == 166


def test_every_parameter_and_return_type_has_the_class_the_header_gives_it():
    declared = prototypes()
    wrong = []
    for name, (restype, argtypes) in bmx.SIGNATURES.items():
        have = (ctypes_class(restype, name), [ctypes_class(t, name) for t in argtypes])
        if have != declared[name]:
            wrong.append((name, have, declared[name]))
    assert not wrong, wrong


def test_the_table_and_the_export_lists_name_the_same_functions():
    assert len(bmx.ALL_EXPORTS) == len(set(bmx.ALL_EXPORTS))
    assert set(bmx.ALL_EXPORTS) == set(bmx.SIGNATURES)
    lists = [getattr(bmx, n) for n in dir(bmx) if n == "EXPORTS" or n.startswith("EXPORTS_")]
    assert sorted(bmx.ALL_EXPORTS) == sorted(s for li in lists for s in li)          # ALL_EXPORTS leaves no list out
