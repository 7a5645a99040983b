// kitti_parse.hpp -- the grammar of a REGULAR KITTI label / result line and the value of its tokens (include/prcnn_hip.h: the
// PRCNN_PARSE_* section), as host + device functions: the kernels of kitti_parse.hip call them per row, a host program can call
// the very same code.  kitti_annos.parse_texts(device="cpu") restates it in Python; kitti_annos._anno_from_rows is the definition.
#pragma once
#include "../../include/prcnn_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PRCNN_HD __host__ __device__
#else
#define PRCNN_HD
#endif

namespace prcnn {

constexpr int PARSE_MAX_DIGITS = 15;      // significant digits of a token: w < 10^15 < 2^53 is an exact f64
constexpr int PARSE_MAX_POW10 = 22;       // 10^22 is the largest power of ten that is an exact f64
constexpr int PARSE_MAX_EXP_DIGITS = 9;   // digits written behind e / E

PRCNN_HD inline bool parse_is_digit(unsigned char c) { return c >= '0' && c <= '9'; }

// [+-]?[0-9]{1,15} -> the integer as f64 (int("-0") is 0: no sign on a zero)
PRCNN_HD inline bool parse_int_token(const unsigned char *s, int len, double *out)
{
    int p = 0;
    const bool neg = len > 0 && s[0] == '-';
    if (len > 0 && (s[0] == '+' || s[0] == '-')) p = 1;
    const int nd = len - p;
    if (nd < 1 || nd > PARSE_MAX_DIGITS) return false;
    long long w = 0;
    for (; p < len; ++p) {
        if (!parse_is_digit(s[p])) return false;
        w = w * 10 + (s[p] - '0');
    }
    *out = (double)(neg ? -w : w);
    return true;
}

// [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)? with at most 15 digits from the first non-zero one to the last one written
// and a net decimal exponent |k| <= 22 -> w * 10^k or w / 10^-k: ONE correctly rounded operation on two exact operands (the exact
// fast path of decimal -> binary conversion), the sign applied last.
PRCNN_HD inline bool parse_float_token(const unsigned char *s, int len, double *out)
{
    constexpr double P10[PARSE_MAX_POW10 + 1] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    int p = 0;
    const bool neg = len > 0 && s[0] == '-';
    if (len > 0 && (s[0] == '+' || s[0] == '-')) p = 1;
    long long w = 0, nfrac = 0;
    int sig = 0, n_int = 0, n_frac = 0;
    for (; p < len && parse_is_digit(s[p]); ++p, ++n_int) {
        if (sig > 0 || s[p] != '0') ++sig;
        if (sig <= PARSE_MAX_DIGITS) w = w * 10 + (s[p] - '0');
    }
    if (p < len && s[p] == '.') {
        for (++p; p < len && parse_is_digit(s[p]); ++p, ++n_frac) {
            if (sig > 0 || s[p] != '0') ++sig;
            if (sig <= PARSE_MAX_DIGITS) w = w * 10 + (s[p] - '0');
        }
        nfrac = n_frac;
    }
    if (n_int + n_frac < 1 || sig > PARSE_MAX_DIGITS) return false;
    long long e = 0;
    if (p < len && (s[p] == 'e' || s[p] == 'E')) {
        ++p;
        const bool eneg = p < len && s[p] == '-';
        if (p < len && (s[p] == '+' || s[p] == '-')) ++p;
        const int nd = len - p;
        if (nd < 1 || nd > PARSE_MAX_EXP_DIGITS) return false;
        for (; p < len; ++p) {
            if (!parse_is_digit(s[p])) return false;
            e = e * 10 + (s[p] - '0');
        }
        if (eneg) e = -e;
    }
    if (p != len) return false;
    const long long k = e - nfrac;
    if (k > PARSE_MAX_POW10 || k < -PARSE_MAX_POW10) return false;
    const double m = (double)w;
    const double v = k >= 0 ? m * P10[k] : m / P10[-k];
    *out = neg ? -v : v;
    return true;
}

// class code of a name token (lower-cased ASCII against the five names of the split table), -1 otherwise; *is_dc: exactly "DontCare"
PRCNN_HD inline int parse_name_code(const unsigned char *s, int len, bool *is_dc)
{
    const char *names[5] = {"car", "pedestrian", "cyclist", "van", "person_sitting"};
    const char *dc = "DontCare";
    bool same = len == 8;
    for (int i = 0; same && i < 8; ++i) same = s[i] == (unsigned char)dc[i];
    *is_dc = same;
    for (int c = 0; c < 5; ++c) {
        int i = 0;
        for (; i < len && names[c][i]; ++i) {
            const unsigned char ch = (s[i] >= 'A' && s[i] <= 'Z') ? (unsigned char)(s[i] + 32) : s[i];
            if (ch != (unsigned char)names[c][i]) break;
        }
        if (i == len && !names[c][i]) return c;
    }
    return -1;
}

// One line [s, s + len) without its '\n'.  -> the token count (0: nothing but spaces), or -1 when the line is not regular.  A
// regular line writes vals (PRCNN_PARSE_COLS f64, the PRCNN_PARSE_* column order), name (offset in the line, length), code, is_dc.
PRCNN_HD inline int parse_line(const unsigned char *s, long long len, double *vals, int *name, signed char *code, unsigned char *is_dc)
{
    // file token 1 .. 15 -> column: truncated occluded alpha bbox(4) h w l x y z ry score; dimensions are stored l, h, w
    constexpr int COL[16] = {-1, PRCNN_PARSE_TRUNCATED, PRCNN_PARSE_OCCLUDED, PRCNN_PARSE_ALPHA, PRCNN_PARSE_BBOX, PRCNN_PARSE_BBOX + 1,
                             PRCNN_PARSE_BBOX + 2, PRCNN_PARSE_BBOX + 3, PRCNN_PARSE_DIMENSIONS + 1, PRCNN_PARSE_DIMENSIONS + 2,
                             PRCNN_PARSE_DIMENSIONS, PRCNN_PARSE_LOCATION, PRCNN_PARSE_LOCATION + 1, PRCNN_PARSE_LOCATION + 2,
                             PRCNN_PARSE_ROTATION_Y, PRCNN_PARSE_SCORE};
    long long a = 0, b = len;
    for (long long i = 0; i < len; ++i)
        if (s[i] != ' ' && (s[i] < 0x21 || s[i] > 0x7e)) return -1;          // '\r', tab, control bytes, NUL, >= 0x80
    while (a < b && s[a] == ' ') ++a;
    while (b > a && s[b - 1] == ' ') --b;
    if (a == b) return 0;
    int ntok = 0;
    vals[PRCNN_PARSE_SCORE] = 0.0;
    for (long long p = a; p < b;) {
        long long q = p;
        while (q < b && s[q] != ' ') ++q;
        if (q == p || ntok >= 16 || q - p > 0x7fffffff) return -1;             // an empty token (two spaces), a 17th column
        const int tl = (int)(q - p);
        if (ntok == 0) {
            bool dc;
            *code = (signed char)parse_name_code(s + p, tl, &dc);
            *is_dc = dc;
            name[0] = (int)p;
            name[1] = tl;
        } else if (!(ntok == 2 ? parse_int_token(s + p, tl, vals + COL[ntok]) : parse_float_token(s + p, tl, vals + COL[ntok]))) {
            return -1;
        }
        ++ntok;
        p = q + 1;
    }
    return (ntok == 15 || ntok == 16) ? ntok : -1;
}

}  // namespace prcnn
