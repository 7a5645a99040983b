"""The binding is read from include/prcnn_hip.h (_lib.read_header): the reader on small header texts, the derived Structure layouts
against the host C compiler's, the struct-pointer argument types, and the names built from the header's enums.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import pkg, ROOT

STRUCTS = ("prcnn_gather_problem", "prcnn_layer_problem", "prcnn_sa_problem", "prcnn_sn_batch", "prcnn_gt_batch", "prcnn_aug_batch",
           "prcnn_train_batch", "prcnn_rcnn_aug", "prcnn_rcnn_target_args", "prcnn_loss_args")


# ---- (a) the reader
def test_reader_structs_declarators_const_arrays_and_widths():
    L = pkg("_lib")
    abi = L.read_header("""
        /* a comment with int bogus(void); inside */
        #ifndef X_H
        #define X_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define LONG_MACRO(a) \\
            ((a) + 1)
        typedef struct t_rec {
            int n, m; long rows;            // two declarators, one type
            const int *pt_off, *tile_off;
            const long long *off; unsigned long long seed;
            unsigned char flag; unsigned char *bytes;
            float anchor[3]; double d; unsigned int u;
            void *any;
        } t_rec;
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert list(abi.structs) == ["t_rec"] and not abi.functions and not abi.enums
    want = [("n", C.c_int), ("m", C.c_int), ("rows", C.c_long), ("pt_off", C.c_void_p), ("tile_off", C.c_void_p), ("off", C.c_void_p),
            ("seed", C.c_ulonglong), ("flag", C.c_ubyte), ("bytes", C.c_void_p), ("anchor", C.c_float * 3), ("d", C.c_double),
            ("u", C.c_uint), ("any", C.c_void_p)]
    assert abi.structs["t_rec"]._fields_ == want
    assert issubclass(abi.structs["t_rec"], C.Structure)


def test_reader_prototypes_void_and_struct_pointers():
    L = pkg("_lib")
    abi = L.read_header("""
        typedef struct t_a { int n; } t_a;
        typedef struct t_b { const t_a *inner; long long k; } t_b;
        int f_none(void);
        const char *f_text(void);
        int f_mixed(int b, float r, double d, long rows, long long total, const float *xyz, unsigned int *hdr,
                    const unsigned long long *seeds, unsigned char *cls, long long *keep, void *stream);
        int f_struct(int nprob, const t_a *problems, t_b *out, void *stream);
    """)
    A, B = abi.structs["t_a"], abi.structs["t_b"]
    assert abi.functions["f_none"] == (C.c_int, [])
    assert abi.functions["f_text"] == (C.c_char_p, [])
    assert abi.functions["f_mixed"] == (C.c_int, [C.c_int, C.c_float, C.c_double, C.c_long, C.c_longlong] + [C.c_void_p] * 6)
    assert abi.functions["f_struct"] == (C.c_int, [C.c_int, C.POINTER(A), C.POINTER(B), C.c_void_p])
    assert B._fields_ == [("inner", C.POINTER(A)), ("k", C.c_longlong)]


def test_reader_enums_with_and_without_values():
    L = pkg("_lib")
    abi = L.read_header("enum { A = 0, B = 1, C = 2 };\nenum {\n  P = 0, Q, R /* x 3 */, S = 17, T, N_ALL,\n};\nenum { NEG = -2, NEXT };")
    assert abi.enums == {"A": 0, "B": 1, "C": 2, "P": 0, "Q": 1, "R": 2, "S": 17, "T": 18, "N_ALL": 19, "NEG": -2, "NEXT": -1}


@pytest.mark.parametrize("text", [
    "int f(short a);",                                  # a type outside the map
    "int f(unsigned a);",
    "int f(int **a);",                                  # pointer to pointer
    "int f(float *const x);",
    "int f(int a[3]);",                                 # an array parameter
    "int f(int);",                                      # no name
    "int f();",
    "int f(int a, ...);",
    "float f(void);",                                   # a return type the library does not use
    "typedef struct t { int x : 3; } t;",               # bit field
    "typedef struct t { struct u *p; } t;",             # a struct the header does not declare
    "typedef struct t { int x; } other;",
    "typedef struct t { int (*fn)(int); } t;",
    "struct t { int x; };",
    "enum E { A };",                                    # a named enum
    "enum { A = B };",
    "enum { A = 1 << 3 };",
    "typedef int handle;",
    "extern int counter;",
    "int f(void) { return 0; }",
])
def test_reader_raises_on_what_it_does_not_know(text):
    L = pkg("_lib")
    with pytest.raises(L.PrcnnError, match="unknown|typedef'd"):
        L.read_header("int before(void);\n" + text + "\nint after(void);")


def test_the_header_itself():
    L = pkg("_lib")
    assert set(STRUCTS) == set(L._abi.structs) and all(L.struct(s) is L._abi.structs[s] for s in STRUCTS)
    assert (L.GatherProblem, L.LayerProblem, L.SaProblem) == tuple(L.struct(s) for s in STRUCTS[:3])
    with pytest.raises(L.PrcnnError):
        L.struct("prcnn_no_such_struct")
    assert L.SIGNATURES["prcnn_nms"] == [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    assert L.SIGNATURES["prcnn_packed_layer_batch"] == [C.c_int, C.POINTER(L.LayerProblem), C.c_int, C.c_void_p]
    assert L._abi.functions["prcnn_last_error"] == (C.c_char_p, [])
    assert type(L.SIGNATURES) is dict and "prcnn_last_error" not in L.SIGNATURES
    assert all(getattr(L, name) == value for name, value in L.ENUMS.items()) and L.ENUMS["PRCNN_CALIB_ROW"] == 35


# ---- (b) layout against the compiler
def test_struct_layouts_match_the_host_compiler(tmp_path):
    L = pkg("_lib")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "prcnn_hip.h"', 'int main(void) {']
    for s in STRUCTS:
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in L.struct(s)._fields_:
            lines.append('    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, name, s, name, s, name))
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    want = []
    for s in STRUCTS:
        T = L.struct(s)
        want.append([s, "sizeof", str(C.sizeof(T))])
        want += [[s, name, str(getattr(T, name).offset), str(getattr(T, name).size)] for name, _ in T._fields_]
    assert got == want
    assert sum(len(L.struct(s)._fields_) for s in STRUCTS) == len(got) - len(STRUCTS) >= 200


# ---- (c) a struct-taking entry takes its own struct only
def test_wrong_struct_is_rejected_before_the_library():
    L = pkg("_lib")
    L.load()
    right = L.struct("prcnn_train_batch")(input_channels=3)         # n_scenes = 0: the entry returns before any launch
    assert L.call("prcnn_train_place", C.byref(right), None) == 0
    wrong = L.struct("prcnn_aug_batch")()
    with pytest.raises(C.ArgumentError):
        L.call("prcnn_train_place", C.byref(wrong), None)
    taking = [name for name, argtypes in L.SIGNATURES.items() if any(hasattr(t, "contents") for t in argtypes)]
    assert len(taking) == 17                                         # 14 batch / args entries and the three *_batch problem lists
    for name in taking:
        with pytest.raises(C.ArgumentError):
            L.call(name, *[C.byref(C.c_double()) if hasattr(t, "contents") else t() for t in L.SIGNATURES[name]])


# ---- (d) names built from the enums
def test_loss_names_follow_the_enums():
    L, losses = pkg("_lib"), pkg("losses")
    lp = {name: value for name, value in L.ENUMS.items() if name.startswith("PRCNN_LP_")}
    assert len(lp) == 24 == losses.PARTS == L.PRCNN_LOSS_PARTS == len(losses.PART_NAMES)
    for name, value in lp.items():
        assert losses.PART_NAMES[value] == name[len("PRCNN_LP_"):].lower() and losses.P[losses.PART_NAMES[value]] == value
    assert losses.PART_NAMES[:6] == ("loss", "cls", "reg", "loc", "angle", "size") and losses.PART_NAMES[-2:] == ("dice_min", "dice_max")
    assert losses.CLS_KINDS == {"DiceLoss": L.PRCNN_LOSS_DICE, "SigmoidFocalLoss": L.PRCNN_LOSS_FOCAL, "BinaryCrossEntropy": L.PRCNN_LOSS_BCE}
    assert (L.PRCNN_LOSS_DICE, L.PRCNN_LOSS_FOCAL, L.PRCNN_LOSS_BCE) == (0, 1, 2)
