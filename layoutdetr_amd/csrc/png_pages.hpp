// What the two device page decoders share: png_decode.hip (stored-block pages) and png_inflate.hip (indexed pages, section 18).
#pragma once
#include "ldetr_common.hpp"

namespace ldetr {

constexpr int PNG_MAX_W = 4096;               // the hand-off row is 3 W bytes of LDS
constexpr int PNG_MAX_H = 32768;
constexpr int PNG_MIN_RANGE = 64;             // rows: an independent row range is at least one band

static inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

#define PNG_MALFORMED(...) do { set_error(__VA_ARGS__); return LDETR_PNG_MALFORMED; } while (0)
#define PNG_NOT_ELIGIBLE(...) do { set_error(__VA_ARGS__); return LDETR_PNG_NOT_ELIGIBLE; } while (0)

// the arguments of png_gather_kernel and png_unfilter_kernel (png_decode.hip)
struct PngParams {
    const uint8_t* files; long files_bytes;        // files_bytes a multiple of 16
    const int64_t* file_off;                       // device [n + 1]
    const int64_t* seg;                            // device [k][4] = (page, offset in file, offset in stream, length)
    long k;
    const int32_t* jobs;                           // device [j][3] = (page, first row, end row)
    uint8_t* stream; long stream_bytes;            // [n][H][1 + 3 W], stream_bytes a multiple of 16 >= n * H * (1 + 3 W)
    uint8_t* dst;                                  // [n][H][W][3]
    int n, H, W;
};

// png_decode.hip: the host-table checks both entries make (LDETR_ERR_ARG with the message prefixed by `who`), and the unfilter launch over a dense stream
// (reads p.jobs, p.stream, p.stream_bytes, p.dst, p.n, p.H, p.W)
int png_check_file_offsets(const char* who, int n, const int64_t* file_off, int64_t files_bytes);
int png_check_jobs(const char* who, int n, int H, const int32_t* jobs, int64_t n_jobs);
int png_launch_unfilter(const PngParams& p, int64_t n_jobs, hipStream_t st, const char* what);

}  // namespace ldetr
