"""Texts for the label / result text parser (helper of test_kitti_parse.py and test_gpu_kitti_parse.py; no test lives here): the
splits the evaluator's tests already use, a seeded sweep over the grammar of a regular number, the catalogue of irregular files, and
the shapes at which the kernels' chunks, waves and line walks meet their ends."""
import functools
import os

import numpy as np

import ap_split

HERE = os.path.dirname(os.path.abspath(__file__))
G10 = os.path.join(HERE, "golden", "g10_ap_eval_ref.npz")
FLOAT_SLOTS = 14                                     # tokens 1 and 3 .. 15 of a 16-token line


def text_of(lines, final_newline=True):
    return "\n".join(lines) + ("\n" if final_newline and lines else "")


@functools.lru_cache(maxsize=None)
def g10_lines():
    z = np.load(G10)
    return [str(s).split("\n") for s in z["gt_lines"]], [str(s).split("\n") for s in z["dt_lines"]]


@functools.lru_cache(maxsize=None)
def sweep_tokens(seed=7, n=2100):
    """>= 2000 tokens of the regular grammar: both signs, the forms D  D.  .D  I.F, leading zeros, 1 .. 15 digits, exponents such that
    the net decimal exponent k covers -22 .. 22, zeros of either sign, and 15-digit values next to 2^53"""
    rng = np.random.RandomState(seed)
    fixed = ["-0.00", "0", "-0", "+0", "0.0", "-.0", "0e22", "-0e-22", "0.000e0", "000", "1e22", "1e-22", "-1E+22", "999999999999999",
             "999999999999999e22", "999999999999999e-22", "900719925474099e1", "900719925474100e1", "900719925474099.e1",
             "9.00719925474099e15", "9.00719925474100e15", "562949953421311e4", "281474976710655.e5", "45035996273704.5",
             "0.000000000000001", "00000000000000000001.50", "1.e0", ".5", "5.", "+.5e+01", "-5.E-01", "1e000000005",
             "0.0000000000000000000001", "123456789012345e-15", "0.3", "0.1", "0.7", "2.675", "1.005", "8.41", "1E22"]
    out = list(fixed)
    k_cycle = 0
    while len(out) < n:
        nd = int(rng.randint(1, 16))
        digits = str(rng.randint(1, 10)) + "".join(str(d) for d in rng.randint(0, 10, nd - 1))
        form = int(rng.randint(0, 4))
        if form == 0:
            body, nfrac = digits, 0
        elif form == 1:
            body, nfrac = digits + ".", 0
        elif form == 2:
            body = "." + "0" * int(rng.randint(0, 3)) + digits
            nfrac = len(body) - 1
        else:
            cut = int(rng.randint(0, nd + 1))
            body, nfrac = (digits[:cut] or "0") + "." + digits[cut:], nd - cut
        if rng.rand() < 0.25 and form != 2:
            body = "0" * int(rng.randint(1, 4)) + body
        k = k_cycle % 45 - 22                            # every k of -22 .. 22, in turn
        k_cycle += 1
        exp = k + nfrac
        if exp != 0 or rng.rand() < 0.5:
            body += "eE"[int(rng.randint(0, 2))] + ("%+d" % exp if rng.rand() < 0.5 else "%d" % exp if rng.rand() < 0.7 else "%+03d" % exp)
        out.append(["", "-", "+"][int(rng.randint(0, 3))] + body)
    return out


def sweep_lines():
    toks = sweep_tokens()
    assert len(toks) % FLOAT_SLOTS == 0 and len(toks) >= 2000
    names = ["Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare", "car", "CAR", "dontcare", "Tram", "Misc", "PERSON_SITTING",
             "Cars", "Ca", "DontCare_", "x" * 40]
    ints = ["0", "1", "2", "3", "-1", "+2", "007", "-0", "999999999999999", "-999999999999999"]
    lines = []
    for r in range(len(toks) // FLOAT_SLOTS):
        t = toks[r * FLOAT_SLOTS:(r + 1) * FLOAT_SLOTS]
        lines.append(" ".join([names[r % len(names)], t[0], ints[r % len(ints)]] + t[1:]))
    return lines


@functools.lru_cache(maxsize=None)
def regular_sides():
    """name -> list of texts (one per file), all inside the regular grammar"""
    g10_gt, g10_dt = g10_lines()
    gl, dl = ap_split.make_split(0)
    sweep = sweep_lines()
    row15 = "Car 0.00 0 -1.57 1.5 2.5 3.5 4.5 1.5 1.6 3.9 -0.00 1.6 12.25 0.5"
    return {
        "g10_gt": [text_of(l, False) for l in g10_gt],
        "g10_dt": [text_of(l, False) for l in g10_dt],
        "split_gt": [text_of(l) for l in gl],
        "split_dt": [text_of(l, i % 2 == 0) for i, l in enumerate(dl)],
        "sweep": [text_of(sweep[i:i + 25], i % 50 == 0) for i in range(0, len(sweep), 25)],
        "cols15_and_16": [row15 + "\n" + row15, row15 + " 0.25\n" + row15 + " -1e-3\n", "", "  " + row15 + "  \n"],
        "only_empty": ["", "", ""],
        "empty_split": [],
    }


ROW = "Car 0.50 1 -1.57 10.5 20.25 30.125 40 1.5 1.6 3.9 -0.00 1.6 12.25 0.5 0.75"
OTHER = "Van 0 2 0.1 1 2 3 4 2.0 1.9 5.0 3 1.5 20 -0.2 1.5"


def _with(index, token, row=ROW):
    toks = row.split(" ")
    toks[index] = token
    return " ".join(toks)


# name -> (text of the file, skip_blank).  Every one is outside the regular grammar: the host parser reads it, or raises.
IRREGULAR = {
    "17_columns": (ROW + " 9.5\n" + OTHER + " 1\n", False),
    "mixed_16_then_15": (ROW + "\n" + " ".join(OTHER.split(" ")[:15]) + "\n", False),
    "mixed_15_then_16": (" ".join(ROW.split(" ")[:15]) + "\n" + OTHER + "\n", False),
    "14_columns": (" ".join(ROW.split(" ")[:14]) + "\n", False),
    "double_space": (ROW.replace(" 1.6 ", "  1.6 ", 1) + "\n", False),
    "double_space_front": (ROW.replace("Car ", "Car  ", 1) + "\n", False),
    "nan": (_with(3, "nan") + "\n", False),
    "inf": (_with(15, "-inf") + "\n" + OTHER + "\n", False),
    "infinity": (_with(4, "Infinity") + "\n", False),
    "underscore": (_with(4, "1_0.5") + "\n", False),
    "16_digits": (_with(5, "0.1234567890123456") + "\n", False),
    "17_digits_integer": (_with(5, "12345678901234567") + "\n", False),
    "16_digits_trailing_zeros": (_with(5, "1.000000000000000") + "\n", False),
    "exponent_23": (_with(6, "1e23") + "\n", False),
    "exponent_minus_23": (_with(6, "1e-23") + "\n", False),
    "net_exponent_minus_23": (_with(6, "0.00000000000000000000001") + "\n", False),
    "exponent_10_digits": (_with(6, "1e0000000001") + "\n", False),
    "huge_exponent": (_with(6, "1e400") + "\n", False),
    "occluded_1.0": (_with(2, "1.0") + "\n", False),
    "occluded_16_digits": (_with(2, "1234567890123456") + "\n", False),
    "occluded_underscore": (_with(2, "1_0") + "\n", False),
    "bare_dot": (_with(7, ".") + "\n", False),
    "bare_exponent": (_with(7, "e5") + "\n", False),
    "dangling_exponent": (_with(7, "1e") + "\n", False),
    "hex": (_with(7, "0x10") + "\n", False),
    "two_signs": (_with(7, "+-1") + "\n", False),
    "tab_separator": (ROW.replace(" ", "\t", 1) + "\n", False),
    "trailing_tab": (ROW + "\t\n" + OTHER + "\n", False),
    "crlf": (ROW + "\r\n" + OTHER + "\r\n", False),
    "lone_cr": (ROW + "\r" + OTHER + "\n", False),
    "utf8_name": (_with(0, "Cär") + "\n", False),
    "nul_byte": (ROW + "\x00\n", False),
    "blank_line": (ROW + "\n\n" + OTHER + "\n", False),
    "blank_line_last": (ROW + "\n   \n", False),
    "newline_only": ("\n", False),
    "skip_blank_but_nan": ("\n" + _with(3, "nan") + "\n\n", True),
    "skip_blank_but_14": (" ".join(ROW.split(" ")[:14]) + "\n\n", True),
}
# regular under skip_blank: blank lines are dropped, nothing goes to the host
BLANKS_DROPPED = ["\n" + ROW + "\n\n   \n" + OTHER + "\n \n", "\n\n", " ", ROW + "\n\n" + OTHER]


def _padded(lines, ends):
    """lines, each padded with leading spaces so that it ENDS (its '\\n', or the file's end for the last) at the byte offsets ``ends``"""
    out, pos = [], 0
    for line, end in zip(lines, ends):
        pad = end - pos - len(line)
        assert pad >= 0, (line, end, pos)
        out.append(" " * pad + line)
        pos = end + 1
    return out


@functools.lru_cache(maxsize=None)
def boundary_sides():
    """name -> (texts, skip_blank): the smallest shapes at which a chunk (4096 bytes), a thread's 16 bytes, a wave's 64 or a line
    walk can go wrong"""
    short = "Car 0 0 0 1 2 3 4 1 1 1 0 0 9 0"                    # 31 bytes
    out = {}
    for final in (False, True):                                  # line ends at 63 64 65, 127 128 129, 255 256 257; so does the file
        for shift in (0, 1, 2):
            ends = [63 + shift, 127 + shift, 255 + shift]
            lines = _padded([short] * 3, ends)
            out["ends_%d_%s" % (shift, "nl" if final else "eof")] = ([text_of(lines, final)] + [text_of([OTHER])] * 2, False)
    for n_files in (1, 2, 65, 300):
        out["files_%d" % n_files] = ([text_of([_with(15, "%d.5" % f), OTHER][:1 + f % 2], f % 3 != 0) for f in range(n_files)], False)
    out["files_300_with_empty"] = ([text_of([_with(15, "%d.5" % f)] * (f % 4), f % 3 != 0) for f in range(300)], False)
    out["only_empty_65"] = ([""] * 65, False)
    out["rows_300"] = ([text_of([_with(15, "%d.25" % r) for r in range(300)])], False)          # > 4 chunks, one file
    out["long_name"] = ([text_of([_with(0, "N" * 300), OTHER]), text_of([_with(0, "Car" + "x" * 4200)], False)], False)
    out["last_token_ends_buffer"] = ([text_of([OTHER]), text_of([_with(15, "0.125")], False)], False)
    # lines that start at the last byte of a chunk and at the first; files that start at a chunk's first byte
    out["chunk_edges"] = ([text_of(_padded([ROW, ROW, OTHER, ROW], [4094, 2 * 4096 - 1, 2 * 4096 + 200, 3 * 4096 - 1])),
                           text_of(_padded([OTHER], [4096 - 1])), text_of([ROW])], False)
    out["exact_chunk"] = ([text_of(_padded([ROW], [4096 - 1]))], False)                       # n_bytes = 4096
    out["chunk_less_one"] = ([text_of(_padded([ROW], [4096 - 1]), False)], False)             # n_bytes = 4095, no final newline
    out["blank_runs"] = (BLANKS_DROPPED + [" " * 5000 + "\n" + ROW], True)
    return out


def host_side(KA, texts, skip_blank=False):
    """the definition: SplitSide of the host parser's dicts"""
    return KA.SplitSide([KA._host_anno(t, skip_blank) for t in texts])


SIDE_ARRAYS = ("off", "off32", "code", "is_dc", "occluded", "truncated", "alpha", "bbox", "location", "dimensions", "rotation_y", "score",
               "box3d", "bev")


def bits(a):
    """dtype, shape and bytes: the sign of a zero and the payload of a NaN count"""
    a = np.ascontiguousarray(a)
    return str(a.dtype), a.shape, a.tobytes()


def assert_same_side(got, want, what=""):
    assert got.n_img == want.n_img, what
    for key in SIDE_ARRAYS:
        assert bits(getattr(got, key)) == bits(getattr(want, key)), (what, key)


def assert_same_annos(got, want, what=""):
    assert len(got) == len(want), what
    for f, (a, b) in enumerate(zip(got, want)):
        assert list(a) == list(b), (what, f)
        for key in a:
            assert bits(a[key]) == bits(b[key]), (what, f, key)
