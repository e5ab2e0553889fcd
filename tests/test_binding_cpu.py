"""CPU tests of the binding's header reader: every declared function gets a prototype of the header's arity, a header the reader cannot
classify raises, the ctypes mirrors, the record dtypes and the constants equal what the C++ compiler makes of the same headers, typed host
pointers are still checked while device addresses pass as integers, and every *_params builder accepts and rejects what it did before the
prototypes were read from the headers."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
B = pkg.binding
HEADERS = (B.HEADER, B.DEBUG_HEADER)


@pytest.fixture(scope="module", autouse=True)
def _library(pkg):
    """the session's package fixture builds the native library where it is missing"""
    return pkg


def _stripped(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


# ---- 1. coverage
def test_reader_finds_every_function_an_independent_regex_finds():
    for debug in (True, False):
        names = set()
        for h in HEADERS if debug else HEADERS[:1]:
            names |= set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", _stripped(h)))
        assert B.declared_symbols(debug) == sorted(names)
        assert sorted(fn for fn, p in B.ABI.protos.items() if debug or p[0] == B.HEADER) == sorted(names)
    assert len(B.declared_symbols()) >= 215


def test_every_exported_function_has_the_headers_arity_and_a_restype():
    L = B.lib(); text = "\n".join(_stripped(h) for h in HEADERS); seen = 0
    for fn in B.declared_symbols():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % fn, text)
        arity = 0 if m.group(1).strip() == "void" else m.group(1).count(",") + 1
        assert hasattr(L, fn), fn                          # the library built from this tree exports all of them
        f = getattr(L, fn)
        assert f.argtypes is not None and len(f.argtypes) == arity, (fn, f.argtypes, arity)
        assert f.restype in (C.c_int, C.c_int64, C.c_char_p, C.c_void_p), (fn, f.restype)
        seen += 1
    assert seen == len(B.PROTOTYPES)
    assert L.gs_last_error.restype is C.c_char_p and L.gs_linearize_bytes.restype is C.c_int64 and L.gs_slam_graph.restype is C.c_void_p


@pytest.mark.parametrize("text", ["int gs_x(size_t n);", "int gs_x(gs_graph *g, unsigned int n);", "typedef struct gs_a { wchar_t x; } gs_a;",
                                  "typedef struct gs_a { double v[GS_NOT_DEFINED]; } gs_a;", "static int gs_counter;", "int gs_x(int a)",
                                  "#define GS_HALF 0.5", "typedef int gs_int;"])
def test_a_declaration_the_reader_cannot_classify_raises_with_its_line(text):
    with pytest.raises(B.cheader.HeaderError, match=r"t\.h:3: "):
        B.cheader.Abi().read("/* a\n comment */\n" + text + "\n", "t.h")


def test_a_pointer_to_a_struct_without_a_mirror_raises():
    a = B.cheader.Abi(); a.read("typedef struct gs_a { double v[2 * 3]; int32_t n, m; } gs_a;\nint gs_x(const gs_a *a, double *dev_out);")
    assert a.structs["gs_a"] == [("v", "double", 6), ("n", "int32_t", None), ("m", "int32_t", None)]
    with pytest.raises(B.cheader.HeaderError):
        a.prototype("gs_x")
    A = a.structure("A", "gs_a")
    assert a.prototype("gs_x") == (C.c_int, [C.POINTER(A), C.c_void_p])


# ---- 2. layouts and constants against the compiler
@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{"S": {struct: size}, "F": {(struct, field): (offset, size)}, "D": {define: value}} as the C++ compiler sees the two headers"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("layout"); src = d / "layout.cpp"; exe = str(d / "layout")
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "graphslam.h"', '#include "graphslam_debug.h"', "int main() {"]
    for s, fields in B.ABI.structs.items():
        lines.append('    std::printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _, _ in fields:
            lines.append('    std::printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f))
    for k in B.ABI.defines:
        lines.append('    std::printf("D %s %%lld\\n", (long long)(%s));' % (k, k))
    src.write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = {"S": {}, "F": {}, "D": {}}
    for ln in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines():
        w = ln.split()
        if w[0] == "F":
            out["F"][(w[1], w[2])] = (int(w[3]), int(w[4]))
        else:
            out[w[0]][w[1]] = int(w[2])
    return out


def test_mirrors_and_records_have_the_compilers_layout(compiled):
    assert set(B.ABI.mirrors) | set(B.ABI.records) == set(B.ABI.structs) == set(compiled["S"]) and len(compiled["S"]) >= 22
    assert not set(B.ABI.mirrors) & set(B.ABI.records)
    for s, fields in B.ABI.structs.items():
        if s in B.ABI.mirrors:
            cls = B.ABI.mirrors[s]
            assert C.sizeof(cls) == compiled["S"][s], s
            assert len(cls._fields_) == len(fields)
            for (f, _, _), (py, _) in zip(fields, cls._fields_):
                assert py == ("lambda_" if f == "lambda" else f)
                assert (getattr(cls, py).offset, getattr(cls, py).size) == compiled["F"][(s, f)], (s, f)
        else:
            d = B.ABI.records[s]
            assert d.itemsize == compiled["S"][s] and d.names == tuple(f for f, _, _ in fields), s
            for f, _, _ in fields:
                assert (d.fields[f][1], d.fields[f][0].itemsize) == compiled["F"][(s, f)], (s, f)
    assert (B.FOLLOW_STATE, B.FOLLOW_STEP, B.CAND, B.CAND_STEP, B.DUP_INFO) == tuple(
        B.ABI.records[s] for s in ("gs_follow_state", "gs_follow_step", "gs_cand", "gs_cand_step", "gs_dup_info"))
    assert B.ABI.mirrors["gs_stats"] is B.Stats and B.ABI.mirrors["gs_config"] is B.Config and B.ABI.mirrors["gs_lm_info"] is B.LmInfo


def test_constants_have_the_compilers_values(compiled):
    assert B.ABI.defines == compiled["D"]
    D = compiled["D"]
    for py in ("NN_FRAME_MAX", "LOC_ITER_MAX", "RELOC_SEED_MAX", "FOLLOW_HYP_MAX", "CAND_MAX", "DUP_MAP_MAX"):
        assert getattr(B, py) == D["GS_" + py]
    assert B.GS_OK == D["GS_OK"] == 0
    assert B.ERRORS == {v: k for k, v in D.items() if k.startswith("GS_ERR_")} and len(B.ERRORS) >= 11
    assert B.ROBUST_KERNELS == {"none": D["GS_ROBUST_NONE"], "huber": D["GS_ROBUST_HUBER"], "cauchy": D["GS_ROBUST_CAUCHY"]}
    assert B.EDGE_KINDS == {"odometry": D["GS_EDGE_ODOMETRY"], "observation": D["GS_EDGE_OBSERVATION"]}
    assert [D["GS_DOGLEG_" + k] for k in B.DOGLEG_KINDS] == [0, 1, 2]
    assert C.sizeof(B.JcParams) == 16 + 8 * (D["GS_NN_FRAME_MAX"] + 1)


# ---- 3. what the prototypes still check
def test_typed_host_pointers_are_checked_and_device_addresses_pass_as_integers():
    G = pkg.Graph(device=-2); L = B.lib()
    try:
        wrong = np.zeros(3, dtype=np.int32)
        with pytest.raises(C.ArgumentError):
            L.gs_add_pose(G.h, 0, wrong.ctypes.data_as(C.POINTER(C.c_int32)))
        with pytest.raises(C.ArgumentError):
            L.gs_get_poses(G.h, 0, np.zeros(1).ctypes.data_as(C.POINTER(C.c_double)), None)
        assert L.gs_add_pose(G.h, 0, np.zeros(3).ctypes.data_as(C.POINTER(C.c_double))) == 0
        # dev_ parameters are c_void_p: a plain integer address goes through (a host-only handle refuses the call before it reads any)
        assert L.gs_associate_resident(G.h, 1, 4096, 1, 4096, 4096, 1.0, 1e-4, 4096) == -4
        assert L.gs_associate_resident.argtypes[2] is C.c_void_p and L.gs_cand_set.argtypes[2] is C.c_void_p
        assert L.gs_dist_unique_id.argtypes == [C.c_char_p] and L.gs_dist_comm_init.argtypes[1] is C.c_char_p
    finally:
        G.close()


# ---- 4. the parameter builders: (builder, struct, fields it sets, names it refuses, what refusing raises) as before the table
BUILDERS = [
    ("nn_params", "NnParams", ("struct_size", "reserved", "gate_chi2", "max_distance", "type_tol", "sigma_range", "sigma_bearing", "sigma_xy"), ("nope",), KeyError),
    ("loc_params", "LocParams", ("max_iterations", "tol_xy", "tol_theta"), ("nope", "struct_size"), AttributeError),
    ("reloc_params", "RelocParams", ("struct_size", "seed_obs", "min_inliers", "min_baseline", "length_tol", "inlier_radius", "type_tol", "distinct_xy", "distinct_cos"),
     ("nope", "reserved"), AttributeError),
    ("follow_params", "FollowParams", ("min_pairs", "max_misses", "merge_xy", "merge_theta"), ("nope", "reserved", "struct_size"), AttributeError),
    ("cand_params", "CandParams", ("confirm_hits", "max_misses", "spawn_range", "view_range", "view_cos"), ("nope", "reserved", "struct_size"), AttributeError),
    ("dup_params", "DupParams", ("require_same_type", "exclusive", "gate_chi2", "max_distance", "sigma_floor"), ("nope", "reserved", "struct_size"), AttributeError),
    ("lm_params", "LmParams", ("max_trials_after_failure", "initial_lambda", "tau"), ("nope", "struct_size"), AttributeError),
    ("dogleg_params", "DoglegParams", ("max_trials_after_failure", "initial_delta"), ("nope", "struct_size"), AttributeError)]


@pytest.mark.parametrize("name,struct,fields,refused,error", BUILDERS, ids=[b[0] for b in BUILDERS])
def test_builder_accepts_its_fields_and_refuses_the_rest(name, struct, fields, refused, error):
    build = getattr(B, name); cls = getattr(B, struct)
    base = build()
    assert type(base) is cls and base.struct_size == C.sizeof(cls)
    for f in fields:
        p = build(**{f: 3})
        assert getattr(p, f) == 3
        for g, _ in cls._fields_:
            if g != f:
                assert getattr(p, g) == getattr(base, g), (f, g)
    for f in refused:
        with pytest.raises(error) as e:
            build(**{f: 3})
        assert type(e.value) is error
    if "max_trials_after_failure" in fields:
        assert build(max_trials=7).max_trials_after_failure == 7


def test_jc_params_default_and_confidence():
    p = B.jc_params(); q = B.jc_params(0.9)
    assert type(p) is B.JcParams and p.confidence == 0.95 and q.confidence == 0.9 and len(p.gate) == B.NN_FRAME_MAX + 1
    assert 0 < q.gate[1] < p.gate[1] < p.gate[2]
    with pytest.raises(B.GsError):
        B.jc_params(1.5)
