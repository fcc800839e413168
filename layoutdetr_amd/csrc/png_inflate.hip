// Page PNGs with COMPRESSED deflate blocks decoded on the device: the files csrc/png_encode.hip writes with an index.
// A general zlib stream is one serial bit stream.  The encoder's files are not: every 64 KiB segment of the filtered scanline stream is its own byte-aligned
// IDAT chunk holding one stored, fixed or dynamic block that no match leaves, inside a segment no token crosses a 512-byte sub-block, and the ancillary ldIX
// chunk in front of the first IDAT publishes where each sub-block's first token starts (big-endian: version 1, segment bytes, sub-block bytes, the filter
// type of every row, then one bit offset per sub-block counted from the first data byte of the segment's chunk; all 0 for a stored segment).  So inflate is
// 128-way parallel inside a segment and segment-parallel across a page.
//
// ldetr_png_scan_packed (HOST memory, no GPU work) accepts exactly that layout and returns the segment table; ldetr_png_inflate_u8 runs at most two launches
// for any number of pages of one size: png_inflate_kernel, one workgroup of 128 lanes per (page, segment) with the output segment in LDS (the kernel body
// and its error model: png_inflate_kernel.hpp), then png_decode.hip's png_unfilter_kernel over the dense stream.  No workgroup waits for another one, there
// are no flags in global memory; the per-page status word is written with plain stores by the workgroups that found an error.
// Adler-32 and the chunk CRC-32s are not checked here (scan_png(verify=True) checks them on the host).
#include <algorithm>
#include <atomic>

#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"
#include "png_pages.hpp"
#include "png_inflate_kernel.hpp"

namespace ldetr {

constexpr int PI_VERSION = 1;

__global__ void __launch_bounds__(PI_THREADS) png_inflate_kernel(PngInflateParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char png_inflate_lds[];
    png_inflate_segment(*reinterpret_cast<PngInflateShared*>(png_inflate_lds), p, (long)blockIdx.y, (long)blockIdx.x);
}

static inline int64_t pi_entries(int64_t total) { return (total / PI_SEG) * PI_NSUB + (total % PI_SEG + PI_SUB - 1) / PI_SUB; }

// bits [at, at + n) of a byte string, LSB first (n <= 16; the caller checked the length)
static inline unsigned pi_bits(const uint8_t* z, int64_t at, int n) {
    unsigned v = 0;
    for (int i = 0; i < n; i++) v |= (unsigned)((z[(at + i) >> 3] >> ((at + i) & 7)) & 1) << i;
    return v;
}

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_png_scan_packed(const uint8_t* file, int64_t file_bytes, int* width, int* height, int64_t* segments, int64_t segments_capacity, int64_t* segments_count,
                                     int64_t* index_offset, int32_t* row_starts, int64_t row_starts_capacity, int64_t* row_starts_count) {
    LDETR_CHECK(file && file_bytes >= 0 && width && height && segments_count && index_offset, "png_scan_packed: bad arguments");
    LDETR_CHECK(segments_capacity >= 0 && row_starts_capacity >= 0, "png_scan_packed: negative capacity");
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (file_bytes < 8) PNG_MALFORMED("png_scan_packed: truncated file (%ld bytes, no signature)", (long)file_bytes);
    if (memcmp(file, sig, 8) != 0) PNG_MALFORMED("png_scan_packed: bad signature");
    // chunks
    int64_t pos = 8, n_idat = 0, first_idat = -1, ix_off = -1, ix_len = 0;
    bool have_ihdr = false, have_iend = false, ix_late = false;
    uint32_t W = 0, H = 0;
    int depth = 0, ctype = 0, interlace = 0;
    while (pos < file_bytes) {
        if (file_bytes - pos < 12) PNG_MALFORMED("png_scan_packed: truncated file (chunk header at byte %ld)", (long)pos);
        const int64_t len = be32(file + pos);
        const uint8_t* type = file + pos + 4;
        if (len > file_bytes - pos - 12) PNG_MALFORMED("png_scan_packed: chunk %.4s at byte %ld: length %ld reaches past the end of the file", (const char*)type, (long)pos, (long)len);
        if (!have_ihdr) {
            if (memcmp(type, "IHDR", 4) != 0 || len != 13) PNG_MALFORMED("png_scan_packed: the first chunk is not a 13-byte IHDR");
            const uint8_t* d = file + pos + 8;
            W = be32(d); H = be32(d + 4); depth = d[8]; ctype = d[9]; interlace = d[12];
            if (W == 0 || H == 0 || W > 0x7fffffffu || H > 0x7fffffffu) PNG_MALFORMED("png_scan_packed: IHDR size %u x %u", W, H);
            if (d[10] != 0 || d[11] != 0 || interlace > 1) PNG_MALFORMED("png_scan_packed: IHDR compression %d / filter %d / interlace %d", d[10], d[11], interlace);
            have_ihdr = true;
        } else if (memcmp(type, "IDAT", 4) == 0) {
            if (first_idat < 0) first_idat = pos;
            n_idat++;
        } else if (memcmp(type, "ldIX", 4) == 0) {
            if (first_idat >= 0 || ix_off >= 0) ix_late = true;
            else { ix_off = pos + 8; ix_len = len; }
        } else if (memcmp(type, "IEND", 4) == 0) {
            have_iend = true;
            break;
        }
        pos += 12 + len;
    }
    if (!have_ihdr) PNG_MALFORMED("png_scan_packed: truncated file (no IHDR)");
    if (!have_iend) PNG_MALFORMED("png_scan_packed: no IEND chunk");
    *width = (int)W; *height = (int)H;
    if (interlace || ctype != 2 || depth != 8) PNG_NOT_ELIGIBLE("png_scan_packed: not an 8-bit RGB, non-interlaced page (colour type %d, %d bits, interlace %d)", ctype, depth, interlace);
    if (W > (uint32_t)PNG_MAX_W || H > (uint32_t)PNG_MAX_H) PNG_NOT_ELIGIBLE("png_scan_packed: %u x %u is larger than the device path takes (%d x %d)", W, H, PNG_MAX_W, PNG_MAX_H);
    if (ix_off < 0 || ix_late) PNG_NOT_ELIGIBLE("png_scan_packed: no ldIX chunk in front of the first IDAT");
    const int64_t stride = 1 + 3 * (int64_t)W, total = stride * (int64_t)H, nseg = (total + PI_SEG - 1) / PI_SEG, entries = pi_entries(total);
    // the index
    if (ix_len < 12) PNG_MALFORMED("png_scan_packed: truncated ldIX chunk (%ld bytes)", (long)ix_len);
    const uint8_t* ix = file + ix_off;
    if (be32(ix) != (uint32_t)PI_VERSION || be32(ix + 4) != (uint32_t)PI_SEG || be32(ix + 8) != (uint32_t)PI_SUB)
        PNG_NOT_ELIGIBLE("png_scan_packed: ldIX version %u with %u-byte segments and %u-byte sub-blocks; this library reads version %d, %d, %d", be32(ix), be32(ix + 4), be32(ix + 8), PI_VERSION,
                         PI_SEG, PI_SUB);
    if (ix_len != 12 + (int64_t)H + 4 * entries) PNG_MALFORMED("png_scan_packed: ldIX chunk of %ld bytes, a %u x %u page has %ld", (long)ix_len, W, H, (long)(12 + (int64_t)H + 4 * entries));
    if (n_idat != nseg) PNG_NOT_ELIGIBLE("png_scan_packed: %ld IDAT chunks, one per 64 KiB segment would be %ld", (long)n_idat, (long)nseg);
    int64_t nrow = 0, last_start = 0;
    for (int64_t y = 0; y < (int64_t)H; y++) {
        const uint8_t fb = ix[12 + y];
        if (fb > 4) PNG_MALFORMED("png_scan_packed: the index gives row %ld the filter byte %d", (long)y, fb);
        if (y == 0 || (fb <= 1 && y - last_start >= PNG_MIN_RANGE)) {                  // the rule of ldetr_png_scan
            if (row_starts && nrow < row_starts_capacity) row_starts[nrow] = (int32_t)y;
            nrow++;
            last_start = y;
        }
    }
    // the segments: IDAT i holds segment i
    const uint8_t* ent = ix + 12 + H;
    pos = first_idat;
    for (int64_t s = 0; s < nseg; s++) {
        const int64_t len = be32(file + pos);
        if (memcmp(file + pos + 4, "IDAT", 4) != 0) PNG_NOT_ELIGIBLE("png_scan_packed: the IDAT chunks are not consecutive");
        const uint8_t* d = file + pos + 8;
        const bool last = s == nseg - 1;
        const int64_t zoff = s == 0 ? 2 : 0, n = last ? total - s * PI_SEG : PI_SEG, nsub = (n + PI_SUB - 1) / PI_SUB;
        const int64_t zl = len - zoff - (last ? 4 : 0);                                 // deflate bytes
        if (zl < 1) PNG_MALFORMED("png_scan_packed: IDAT chunk %ld of %ld bytes holds no deflate block", (long)s, (long)len);
        if (s == 0) {
            const uint8_t cmf = d[0], flg = d[1];
            if ((cmf & 0x0f) != 8 || (cmf >> 4) > 7 || (((unsigned)cmf << 8) | flg) % 31 != 0) PNG_MALFORMED("png_scan_packed: bad zlib header %02x %02x", cmf, flg);
            if (flg & 0x20) PNG_NOT_ELIGIBLE("png_scan_packed: zlib stream with a preset dictionary");
        }
        const uint8_t* z = d + zoff;
        const int btype = (z[0] >> 1) & 3;
        const uint8_t* e = ent + 4 * (s * PI_NSUB);
        if (btype == 3) PNG_MALFORMED("png_scan_packed: deflate block of reserved type 3");
        if (btype == 0) {
            const int64_t nb = (n + 65534) / 65535;
            if (zl != n + 5 * nb) PNG_NOT_ELIGIBLE("png_scan_packed: segment %ld: %ld deflate bytes, its stored form has %ld", (long)s, (long)zl, (long)(n + 5 * nb));
            for (int64_t b = 0; b < nb; b++) {
                const uint8_t* h = z + b * 65540;
                const unsigned blen = h[1] | ((unsigned)h[2] << 8), nlen = h[3] | ((unsigned)h[4] << 8);
                if ((blen ^ nlen) != 0xffffu) PNG_MALFORMED("png_scan_packed: stored block with LEN %04x, NLEN %04x (not its complement)", blen, nlen);
                if ((h[0] & 6) != 0 || (h[0] & 1) != ((last && b == nb - 1) ? 1 : 0) || (int64_t)blen != std::min<int64_t>(65535, n - b * 65535))
                    PNG_NOT_ELIGIBLE("png_scan_packed: segment %ld is not in the stored form (block %ld)", (long)s, (long)b);
            }
            for (int64_t k = 0; k < nsub; k++)
                if (be32(e + 4 * k) != 0) PNG_NOT_ELIGIBLE("png_scan_packed: stored segment %ld with a non-zero index entry", (long)s);
        } else {
            if (z[0] & 1) PNG_NOT_ELIGIBLE("png_scan_packed: segment %ld: the compressed block is final (no empty stored block behind it)", (long)s);
            if (zl < 5 || z[zl - 4] != 0 || z[zl - 3] != 0 || z[zl - 2] != 0xff || z[zl - 1] != 0xff)
                PNG_NOT_ELIGIBLE("png_scan_packed: segment %ld does not end with an empty stored block", (long)s);
            int64_t hdr = 3;
            if (btype == 2) {
                if (zl < 10 + 4) PNG_MALFORMED("png_scan_packed: segment %ld: truncated dynamic block header", (long)s);
                const int hlit = 257 + (int)pi_bits(z, 3, 5), hdist = 1 + (int)pi_bits(z, 8, 5), hclen = (int)pi_bits(z, 13, 4);
                bool flat = hclen == 15 && hlit <= 286 && hdist <= 30;
                for (int k = 0; k < 19 && flat; k++) flat = pi_bits(z, 17 + 3 * k, 3) == (k < 3 ? 0u : 4u);
                if (!flat) PNG_NOT_ELIGIBLE("png_scan_packed: segment %ld: the dynamic block's code lengths are not sent as flat 4-bit codes", (long)s);
                hdr = 17 + 57 + 4 * (hlit + hdist);
            }
            // entries: the first one right behind the header, strictly increasing, all in front of the trailer
            const int64_t lim = 8 * (zoff + zl - 4);
            int64_t prev = -1;
            for (int64_t k = 0; k < nsub; k++) {
                const int64_t v = be32(e + 4 * k);
                if (k == 0 && v != 8 * zoff + hdr) PNG_MALFORMED("png_scan_packed: segment %ld: index entry 0 is bit %ld, the block header ends at bit %ld", (long)s, (long)v, (long)(8 * zoff + hdr));
                if (v <= prev) PNG_MALFORMED("png_scan_packed: segment %ld: index entry %ld (bit %ld) does not lie behind entry %ld (bit %ld)", (long)s, (long)k, (long)v, (long)(k - 1), (long)prev);
                if (v >= lim) PNG_MALFORMED("png_scan_packed: segment %ld: index entry %ld (bit %ld) lies outside the chunk's %ld bits of tokens", (long)s, (long)k, (long)v, (long)lim);
                prev = v;
            }
        }
        if (segments && s < segments_capacity) { segments[4 * s] = pos + 8; segments[4 * s + 1] = len; segments[4 * s + 2] = btype; segments[4 * s + 3] = s * PI_NSUB; }
        pos += 12 + len;
    }
    *segments_count = nseg;
    *index_offset = ix_off;
    if (row_starts_count) *row_starts_count = nrow;
    LDETR_CHECK(!segments || nseg <= segments_capacity, "png_scan_packed: segment table too small (%ld entries, %ld needed)", (long)segments_capacity, (long)nseg);
    LDETR_CHECK(!row_starts || nrow <= row_starts_capacity, "png_scan_packed: row-start table too small (%ld entries, %ld needed)", (long)row_starts_capacity, (long)nrow);
    return LDETR_OK;
}

extern "C" int ldetr_png_inflate_u8(const ldetr_png_inflate_args* a, void* stream) {
    LDETR_CHECK_BLOCK(a, ldetr_png_inflate_args, "png_inflate");
    const int n = a->n, H = a->H, W = a->W;
    LDETR_CHECK(n >= 0 && n <= 65535, "png_inflate: 0 <= pages <= 65535 (got %d)", n);
    if (n == 0) return LDETR_OK;
    LDETR_CHECK(W >= 1 && W <= PNG_MAX_W && H >= 1 && H <= PNG_MAX_H, "png_inflate: page %d x %d outside [1, %d] x [1, %d]", W, H, PNG_MAX_W, PNG_MAX_H);
    LDETR_CHECK((a->phases & ~3) == 0 && a->phases != 0, "png_inflate: phases %d (1 inflate, 2 unfilter, 3 both)", a->phases);
    LDETR_CHECK(a->reserved == 0, "png_inflate: reserved %d", a->reserved);
    LDETR_CHECK(a->files && a->file_off && a->file_off_dev && a->segments && a->segments_dev && a->index_off && a->index_off_dev && a->jobs && a->jobs_dev && a->scratch && a->dst && a->status,
                "png_inflate: null pointer");
    LDETR_CHECK(a->files_bytes > 0 && a->files_bytes % 16 == 0 && ((uintptr_t)a->files & 15) == 0, "png_inflate: the file buffer must be 16-byte aligned and a multiple of 16 bytes long");
    const int64_t stride = 1 + 3 * (int64_t)W, S = stride * H, nseg = (S + PI_SEG - 1) / PI_SEG, entries = pi_entries(S);
    const int64_t need = (n * S + 15) / 16 * 16;
    LDETR_CHECK(((uintptr_t)a->scratch & 15) == 0 && a->scratch_bytes % 16 == 0 && a->scratch_bytes >= need, "png_inflate: scratch must be 16-byte aligned and hold %ld bytes (a multiple of 16; got %ld)",
                (long)need, (long)a->scratch_bytes);
    LDETR_CHECK(((uintptr_t)a->dst & 3) == 0 && ((uintptr_t)a->status & 3) == 0, "png_inflate: dst and status must be 4-byte aligned");
    LDETR_CHECK(a->n_jobs >= n && a->n_jobs <= (int64_t)n * PNG_MAX_H, "png_inflate: %ld row ranges for %d pages", (long)a->n_jobs, n);
    int rc = png_check_file_offsets("png_inflate", n, a->file_off, a->files_bytes);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        const int64_t flen = a->file_off[i + 1] - a->file_off[i], ix = a->index_off[i];
        LDETR_CHECK(a->file_off[i] % 16 == 0, "png_inflate: file %d starts at byte %ld: every file must be 16-byte aligned", i, (long)a->file_off[i]);
        LDETR_CHECK(ix >= 0 && ix <= flen && 12 + (int64_t)H + 4 * entries <= flen - ix, "png_inflate: the index of page %d (offset %ld, %ld bytes) leaves its file of %ld bytes", i, (long)ix,
                    (long)(12 + (int64_t)H + 4 * entries), (long)flen);
        for (int64_t s = 0; s < nseg; s++) {
            const int64_t* q = a->segments + 4 * (i * nseg + s);
            LDETR_CHECK(q[1] >= 1 && q[0] >= 0 && q[0] <= flen && q[1] <= flen - q[0], "png_inflate: page %d segment %ld (offset %ld, length %ld) leaves its file of %ld bytes", i, (long)s, (long)q[0],
                        (long)q[1], (long)flen);
            LDETR_CHECK(q[2] >= 0 && q[2] <= 2 && q[3] == s * PI_NSUB, "png_inflate: page %d segment %ld: kind %ld, first index entry %ld (expected %ld)", i, (long)s, (long)q[2], (long)q[3],
                        (long)(s * PI_NSUB));
        }
    }
    rc = png_check_jobs("png_inflate", n, H, a->jobs, a->n_jobs);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->phases & 1) {
        PngInflateParams p;
        p.files = a->files; p.files_bytes = a->files_bytes; p.file_off = a->file_off_dev; p.seg = a->segments_dev; p.index_off = a->index_off_dev;
        p.stream = a->scratch; p.stream_bytes = a->scratch_bytes; p.status = a->status; p.n = n; p.H = H; p.W = W; p.nseg = nseg; p.total = S;
        // once per device, not per call (the call sits on the training step's host path); per device as in gemm_conv.hip: the attribute belongs to
        // the device's code object
        static std::atomic<bool> raised[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
        if (dev < 0 || !raised[dev].load(std::memory_order_acquire)) {
            LDETR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(png_inflate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PngInflateShared)) == hipSuccess,
                        "png_inflate: the device does not grant %d bytes of LDS per workgroup", (int)sizeof(PngInflateShared));
            if (dev >= 0) raised[dev].store(true, std::memory_order_release);
        }
        hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)nseg, (unsigned)n), PI_THREADS, sizeof(PngInflateShared), st, p);
        rc = check_launch("png_inflate (inflate)");
        if (rc) return rc;
    }
    if (a->phases & 2) {
        PngParams u;
        u.files = a->files; u.files_bytes = a->files_bytes; u.file_off = a->file_off_dev; u.seg = nullptr; u.k = 0; u.jobs = a->jobs_dev;
        u.stream = a->scratch; u.stream_bytes = a->scratch_bytes; u.dst = a->dst; u.n = n; u.H = H; u.W = W;
        return png_launch_unfilter(u, a->n_jobs, st, "png_inflate (unfilter)");
    }
    return LDETR_OK;
}
