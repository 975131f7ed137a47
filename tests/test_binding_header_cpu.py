"""CPU: the ctypes binding (openpano_amd/hip.py) agrees with the C-ABI it binds (include/openpano_hip.h).

1. Prototypes: every ``ret op_name(params);`` of the header, comments stripped, against ``hip.PROTOTYPES`` -- the same set of
   names in both directions, the same number of arguments, and for every argument and return value the ctypes class the
   header's type asks for (a pointer: c_void_p, c_char_p or a POINTER(...); int / int64_t / uint32_t / float / double: c_int /
   c_int64 / c_uint32 / c_float / c_double; a void return: None; a pointer return: c_void_p or c_char_p).  A wrong count or a
   64-bit return left at ctypes' default int otherwise shows only when something misbehaves on a device.
2. Structs: a few lines of C compiled against the header print sizeof and every member's offsetof / sizeof of op_config,
   op_image, op_blend_image and op_blend_geom; OpConfig, OpImage, OpBlendImage and OpBlendGeom must have the same members in the
   same order at the same places.  The member lists are written out here, not read from the Python classes.

Nothing here loads the library or makes a compute call."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from openpano_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openpano_hip.h")

SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double}


def header_prototypes():
    """{name: (return type, [parameter declarations])} of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    protos = {}
    for stmt in re.split(r"[;{}]", text):                       # struct and enum bodies fall apart into statements without "("
        m = re.match(r"\s*(.+?)\b(op_\w+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if not m:
            assert "(" not in stmt, "a statement with a parenthesis that is no op_* prototype: %r" % stmt
            continue
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        assert name not in protos, name
        protos[name] = (ret, [] if params == "void" else [p.strip() for p in params.split(",")])
    return protos


def type_of(decl, named):
    """"pointer", "void" or a key of SCALARS for a parameter declaration (named: its last word is the parameter's name) or a
    return type"""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if named:
        assert len(words) >= 2, "a parameter without a name: %r" % decl
        words = words[:-1]
    kind = " ".join(words)
    assert kind == "void" or kind in SCALARS, "a type this test does not know: %r" % decl
    return kind


def is_pointer_class(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_header_parse_finds_the_abi():
    """the parser itself: the whole header, with the shapes it has to cope with"""
    protos = header_prototypes()
    assert set(protos) == set(re.findall(r"\b(op_[a-z0-9_]+)\s*\(", open(HEADER).read())) and len(protos) > 100
    assert protos["op_abi_version"] == ("int", [])
    assert protos["op_last_error"] == ("const char*", [])
    assert protos["op_features_free"] == ("void", ["op_features* f"])
    assert protos["op_features_from_host"][1][1] == "const float* const* desc"
    assert protos["op_sift_batch_host"][1][6] == "int64_t capacity_rows"
    assert len(protos["op_perspective_homography"][1]) == 13
    assert protos["op_views_decode_jpeg_oriented"][1][4] == "const int* orientation"       # a prototype over two lines
    assert protos["op_ransac_pairs_multi"][1][-1] == "struct op_ransac_result** out"


def test_table_names_equal_header_names():
    protos = header_prototypes()
    assert sorted(set(hip.PROTOTYPES) - set(protos)) == [], "bound, but not in the header"
    assert sorted(set(protos) - set(hip.PROTOTYPES)) == [], "in the header, but not bound"


def test_table_prototypes_match_header():
    bad = []
    for name, (ret, params) in sorted(header_prototypes().items()):
        if name not in hip.PROTOTYPES:
            continue                                            # test_table_names_equal_header_names reports it
        restype, argtypes = hip.PROTOTYPES[name]
        if len(argtypes) != len(params):
            bad.append("%s: %d arguments bound, the header has %d" % (name, len(argtypes), len(params)))
            continue
        kind = type_of(ret, named=False)
        if kind == "void":
            ok = restype is None
        elif kind == "pointer":
            ok = restype in (C.c_void_p, C.c_char_p)
        else:
            ok = restype is SCALARS[kind]
        if not ok:
            bad.append("%s: returns %r, bound as %r" % (name, ret, restype))
        for k, (decl, t) in enumerate(zip(params, argtypes)):
            kind = type_of(decl, named=True)
            assert kind != "void", decl
            if not (is_pointer_class(t) if kind == "pointer" else t is SCALARS[kind]):
                bad.append("%s: argument %d is %r, bound as %r" % (name, k, decl, t))
    assert not bad, "\n".join(bad)


STRUCTS = [
    ("op_config", hip.OpConfig, [
        "SIFT_WORKING_SIZE", "NUM_OCTAVE", "NUM_SCALE", "SCALE_FACTOR", "GAUSS_SIGMA", "GAUSS_WINDOW_FACTOR",
        "JUDGE_EXTREMA_DIFF_THRES", "CONTRAST_THRES", "PRE_COLOR_THRES", "EDGE_RATIO", "CALC_OFFSET_DEPTH", "OFFSET_THRES",
        "ORI_RADIUS", "ORI_HIST_SMOOTH_COUNT", "DESC_HIST_SCALE_FACTOR", "DESC_INT_FACTOR", "MATCH_REJECT_NEXT_RATIO",
        "RANSAC_ITERATIONS", "RANSAC_INLIER_THRES", "INLIER_IN_MATCH_RATIO", "INLIER_IN_POINTS_RATIO", "CYLINDER", "TRANS",
        "ESTIMATE_CAMERA", "ORDERED_INPUT", "LAZY_READ", "MULTIBAND", "MAX_OUTPUT_SIZE", "FOCAL_LENGTH"]),
    ("op_image", hip.OpImage, ["data", "h", "w", "on_device", "dtype"]),
    ("op_blend_image", hip.OpBlendImage, ["data", "h", "w", "on_device", "homo_inv", "range", "mat_h", "mat_w"]),
    ("op_blend_geom", hip.OpBlendGeom, ["proj_method", "proj_min", "proj_max", "resolution"]),
]


def test_struct_layouts_match_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "openpano_hip.h"', "int main(void) {"]
    for cname, _, members in STRUCTS:
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for m in members:
            lines.append('printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, m, cname, m, cname, m))
    lines += ["return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    want = {}
    for line in out:
        w = line.split()
        if len(w) == 3:
            want[w[0]] = int(w[2])
        elif len(w) == 4:
            want[w[0], w[1]] = (int(w[2]), int(w[3]))
    for cname, cls, members in STRUCTS:
        assert [n for n, _ in cls._fields_] == members, cname
        assert C.sizeof(cls) == want[cname], cname
        for m in members:
            field = getattr(cls, m)
            assert (field.offset, field.size) == want[cname, m], (cname, m)
