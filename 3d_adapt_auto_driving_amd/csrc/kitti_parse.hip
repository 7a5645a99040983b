// kitti_parse.hip -- the text of a whole split side (all label or result files, concatenated) to the columns of
// kitti_annos.SplitSide on the device.  The host parser (kitti_annos._anno_from_rows: one Python float() per token) is the
// definition; a regular file (kitti_parse.hpp) gives its bits, an irregular one is flagged and left to the host, whole.
//   scan:   a line starts at the first byte of a non-empty file and behind every '\n' that is not the buffer's last byte.  Line
//           starts are counted per PRCNN_PARSE_CHUNK bytes, the chunk counts are scanned by one workgroup in a fixed order, and one
//           wave per file boundary turns them into the files' row offsets (what the host reads back to size the outputs).
//   rows:   the same count again, now placing every line start at its row; then one thread per row walks its line.
// Integer sums and an integer OR per file only: the same text gives the same bytes.  Every loop is bounded by a chunk, a line or
// the chunk count; every read is below n_bytes, every write below the row / file / chunk count it was sized for.
#include "common.hpp"
#include "kitti_parse.hpp"

namespace prcnn {

constexpr int PARSE_THREADS = 256;
constexpr int PARSE_PER_THREAD = PRCNN_PARSE_CHUNK / PARSE_THREADS;      // 16 consecutive bytes per thread

__device__ __forceinline__ bool parse_line_start(const unsigned char *__restrict__ text, const unsigned char *__restrict__ start_flag,
                                                 long long i)
{
    return start_flag[i] != 0 || (i > 0 && text[i - 1] == '\n');
}

__global__ __launch_bounds__(PARSE_THREADS) void parse_mark_files_kernel(int n_files, const long long *__restrict__ file_off,
                                                                         unsigned char *__restrict__ start_flag)
{
    const int f = blockIdx.x * PARSE_THREADS + threadIdx.x;
    if (f < n_files && file_off[f] < file_off[f + 1]) start_flag[file_off[f]] = 1;
}

// line starts of this thread's 16 bytes, as a bit mask
__device__ __forceinline__ unsigned int parse_thread_starts(long long n_bytes, const unsigned char *__restrict__ text,
                                                            const unsigned char *__restrict__ start_flag, long long base)
{
    unsigned int mask = 0;
#pragma unroll
    for (int j = 0; j < PARSE_PER_THREAD; ++j)
        if (base + j < n_bytes && parse_line_start(text, start_flag, base + j)) mask |= 1u << j;
    return mask;
}

// exclusive scan of one int per thread over the workgroup; *total: the sum
__device__ __forceinline__ int parse_block_excl_scan(int v, int *total)
{
    __shared__ int wave_sum[PARSE_THREADS / WAVE];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int incl = wave_incl_scan(v, lane);
    if (lane == WAVE - 1) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PARSE_THREADS / WAVE; ++w) {
        if (w < wave) before += wave_sum[w];
        all += wave_sum[w];
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(PARSE_THREADS) void parse_count_kernel(long long n_bytes, const unsigned char *__restrict__ text,
                                                                    const unsigned char *__restrict__ start_flag,
                                                                    int *__restrict__ chunk_rows)
{
    const long long base = (long long)blockIdx.x * PRCNN_PARSE_CHUNK + (long long)threadIdx.x * PARSE_PER_THREAD;
    int total;
    parse_block_excl_scan(__popc(parse_thread_starts(n_bytes, text, start_flag, base)), &total);
    if (threadIdx.x == 0) chunk_rows[blockIdx.x] = total;
}

// chunk_rows (n_chunks + 1): counts in, exclusive prefix sums out, the total in the last word.  One workgroup, chunk order.
__global__ __launch_bounds__(PARSE_THREADS) void parse_scan_chunks_kernel(int n_chunks, int *__restrict__ chunk_rows)
{
    int carry = 0;
    for (int c0 = 0; c0 < n_chunks; c0 += PARSE_THREADS) {
        const int c = c0 + (int)threadIdx.x;
        const int v = c < n_chunks ? chunk_rows[c] : 0;
        int total;
        const int excl = parse_block_excl_scan(v, &total);
        if (c < n_chunks) chunk_rows[c] = carry + excl;
        carry += total;
        __syncthreads();                      // wave_sum is written again in the next round
    }
    if (threadIdx.x == 0) chunk_rows[n_chunks] = carry;
}

// row_off[f] = line starts below file_off[f], f = 0 .. n_files: one wave per boundary counts the part of its chunk below it
__global__ __launch_bounds__(PARSE_THREADS) void parse_file_rows_kernel(long long n_bytes, int n_files, const unsigned char *__restrict__ text,
                                                                        const long long *__restrict__ file_off,
                                                                        const unsigned char *__restrict__ start_flag,
                                                                        const int *__restrict__ chunk_rows, long long *__restrict__ row_off)
{
    const int f = blockIdx.x * (PARSE_THREADS / WAVE) + (int)threadIdx.x / WAVE;
    if (f > n_files) return;
    const long long end = file_off[f], chunk = end / PRCNN_PARSE_CHUNK;
    int n = 0;
    for (long long i = chunk * PRCNN_PARSE_CHUNK + lane_id(); i < end; i += WAVE) n += parse_line_start(text, start_flag, i) ? 1 : 0;
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) n += __shfl_xor(n, d, WAVE);
    if (lane_id() == 0) row_off[f] = (long long)chunk_rows[chunk] + n;
}

__global__ __launch_bounds__(PARSE_THREADS) void parse_place_rows_kernel(long long n_bytes, long long n_rows, const unsigned char *__restrict__ text,
                                                                         const unsigned char *__restrict__ start_flag,
                                                                         const int *__restrict__ chunk_rows, int *__restrict__ row_start)
{
    const long long base = (long long)blockIdx.x * PRCNN_PARSE_CHUNK + (long long)threadIdx.x * PARSE_PER_THREAD;
    unsigned int mask = parse_thread_starts(n_bytes, text, start_flag, base);
    int total;
    long long row = (long long)chunk_rows[blockIdx.x] + parse_block_excl_scan(__popc(mask), &total);
    for (; mask; mask &= mask - 1, ++row)
        if (row < n_rows) row_start[row] = (int)(base + __ffs(mask) - 1);
}

// one thread per row: its file (the last one whose rows begin at or below it), its line, the tokens
__global__ __launch_bounds__(PARSE_THREADS) void parse_rows_kernel(long long n_rows, int n_files, int skip_blank, const unsigned char *__restrict__ text,
                                                                   const long long *__restrict__ file_off, const long long *__restrict__ row_off,
                                                                   const int *__restrict__ row_start, double *__restrict__ vals,
                                                                   int *__restrict__ name_span, signed char *__restrict__ code,
                                                                   unsigned char *__restrict__ is_dc, unsigned char *__restrict__ row_tok,
                                                                   int *__restrict__ file_flag)
{
    const long long row = (long long)blockIdx.x * PARSE_THREADS + threadIdx.x;
    if (row >= n_rows) return;
    int lo = 0, hi = n_files;                   // row_off[lo] <= row < row_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (row_off[mid] <= row) lo = mid; else hi = mid;
    }
    const long long begin = row_start[row], file_end = file_off[lo + 1];
    long long end = begin;
    while (end < file_end && text[end] != '\n') ++end;
    double v[PRCNN_PARSE_COLS];
#pragma unroll
    for (int c = 0; c < PRCNN_PARSE_COLS; ++c) v[c] = 0.0;
    int span[2] = {0, 0};
    signed char cls = -1;
    unsigned char dc = 0;
    const int ntok = parse_line(text + begin, end - begin, v, span, &cls, &dc);
    const bool ok = ntok > 0;
#pragma unroll
    for (int c = 0; c < PRCNN_PARSE_COLS; ++c) vals[row * PRCNN_PARSE_COLS + c] = ok ? v[c] : 0.0;
    name_span[2 * row] = ok ? (int)begin + span[0] : 0;
    name_span[2 * row + 1] = ok ? span[1] : 0;
    code[row] = ok ? cls : (signed char)-1;
    is_dc[row] = ok ? dc : (unsigned char)0;
    row_tok[row] = (unsigned char)(ok ? ntok : 0);
    const int flag = ntok == 15 ? PRCNN_PARSE_SAW15 : ntok == 16 ? PRCNN_PARSE_SAW16 : (ntok == 0 && skip_blank) ? 0 : PRCNN_PARSE_BAD;
    if (flag) atomicOr(file_flag + lo, flag);
}

static int parse_check_sizes(long long n_bytes, int n_files, const void *text, const void *file_off)
{
    PRCNN_REQUIRE(n_bytes >= 0 && n_bytes <= PRCNN_PARSE_MAX_BYTES, "kitti_parse: n_bytes %lld is outside [0, 2^31 - 1]", n_bytes);
    PRCNN_REQUIRE(n_files >= 0, "kitti_parse: n_files %d", n_files);
    PRCNN_REQUIRE(file_off && (text || n_bytes == 0), "kitti_parse: null text or file_off");
    return PRCNN_OK;
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_kitti_parse_scan(long long n_bytes, int n_files, const unsigned char *text, const long long *file_off,
                                      unsigned char *start_flag, int *chunk_rows, long long *row_off, void *stream)
{
    if (const int rc = parse_check_sizes(n_bytes, n_files, text, file_off)) return rc;
    PRCNN_REQUIRE(chunk_rows && row_off && (start_flag || n_bytes == 0), "kitti_parse_scan: null output");
    hipStream_t st = (hipStream_t)stream;
    const int n_chunks = ceil_div(n_bytes, PRCNN_PARSE_CHUNK);
    if (n_bytes > 0) {
        PRCNN_REQUIRE(n_files > 0, "kitti_parse_scan: %lld bytes in no file", n_bytes);
        if (hipMemsetAsync(start_flag, 0, (size_t)n_bytes, st) != hipSuccess) return check_launch("kitti_parse_scan: clear");
        parse_mark_files_kernel<<<ceil_div(n_files, PARSE_THREADS), PARSE_THREADS, 0, st>>>(n_files, file_off, start_flag);
        parse_count_kernel<<<n_chunks, PARSE_THREADS, 0, st>>>(n_bytes, text, start_flag, chunk_rows);
    }
    parse_scan_chunks_kernel<<<1, PARSE_THREADS, 0, st>>>(n_chunks, chunk_rows);
    parse_file_rows_kernel<<<ceil_div(n_files + 1, PARSE_THREADS / WAVE), PARSE_THREADS, 0, st>>>(n_bytes, n_files, text, file_off, start_flag,
                                                                                                  chunk_rows, row_off);
    return check_launch("kitti_parse_scan");
}

extern "C" int prcnn_kitti_parse_rows(long long n_bytes, int n_files, long long n_rows, int skip_blank, const unsigned char *text,
                                      const long long *file_off, const unsigned char *start_flag, const int *chunk_rows,
                                      const long long *row_off, int *row_start, double *vals, int *name_span, char *code,
                                      unsigned char *is_dc, unsigned char *row_tok, int *file_flag, void *stream)
{
    if (const int rc = parse_check_sizes(n_bytes, n_files, text, file_off)) return rc;
    PRCNN_REQUIRE(n_rows >= 0 && n_rows <= n_bytes, "kitti_parse_rows: %lld rows in %lld bytes", n_rows, n_bytes);
    PRCNN_REQUIRE(file_flag || n_files == 0, "kitti_parse_rows: null file_flag");
    hipStream_t st = (hipStream_t)stream;
    if (n_files > 0 && hipMemsetAsync(file_flag, 0, sizeof(int) * (size_t)n_files, st) != hipSuccess)
        return check_launch("kitti_parse_rows: clear");
    if (n_rows == 0) return PRCNN_OK;
    PRCNN_REQUIRE(start_flag && chunk_rows && row_off && row_start && vals && name_span && code && is_dc && row_tok,
                  "kitti_parse_rows: null pointer");
    parse_place_rows_kernel<<<ceil_div(n_bytes, PRCNN_PARSE_CHUNK), PARSE_THREADS, 0, st>>>(n_bytes, n_rows, text, start_flag, chunk_rows,
                                                                                           row_start);
    parse_rows_kernel<<<ceil_div(n_rows, PARSE_THREADS), PARSE_THREADS, 0, st>>>(n_rows, n_files, skip_blank, text, file_off, row_off,
                                                                                 row_start, vals, name_span, (signed char *)code, is_dc,
                                                                                 row_tok, file_flag);
    return check_launch("kitti_parse_rows");
}
