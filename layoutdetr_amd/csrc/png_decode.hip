// The page backgrounds of the dataset decoded on the device: PNG files whose zlib stream holds stored blocks only.
// The reference's dataset_tool.py:325-363 saves every PNG with compress_level=0, optimize=False; Pillow then writes a zlib stream of stored
// (BTYPE 00) blocks, so nothing is entropy-coded and the file holds the filtered scanlines as they are, cut into pieces by 5-byte block headers
// and 12 bytes of chunk framing per IDAT chunk.  What dataset_layoutganpp.py:329-340 gets from PIL.Image.open + np.array is then
//     stream [H][1 + 3 W]  = the stored payloads, concatenated           (a copy)
//     page   [H][W][3]     = the PNG row filters undone, row by row      (a scan: recon(x, y) needs recon(x-1, y), recon(x, y-1), recon(x-1, y-1))
//
// ldetr_png_scan (HOST memory, no GPU work) walks the chunks and the zlib stream of one file and returns the table of contiguous payload runs
// (offset in file, offset in stream, length), validates every row's filter byte (so the kernels have no error path) and lists the rows at which an
// independent row range may start: a row with filter 0 (None) or 1 (Sub) never reads the row above.
//
// ldetr_png_decode_u8: at most two launches for any number of pages of one size.
//  (a) png_gather_kernel: one block per payload run (grid-stride), a coalesced copy into the dense stream.  Destination dwords are aligned; the
//      source is read as aligned dwords too and funnel-shifted (v_alignbyte) by the difference of the two alignments, or moved as 16-byte
//      vectors when source and destination agree modulo 16.  Pillow's 65 535-byte blocks in 65 536-byte chunks give every alignment.
//  (b) png_unfilter_kernel: one workgroup of PNG_WAVES waves per (page, independent row range).  A wave owns a band of 64 rows, one row per lane,
//      and runs a skewed wavefront: at step T lane l reconstructs pixel x = T - l of its row, so the pixel above it was produced by lane l - 1 in
//      the step before and arrives with ONE cross-lane move of the packed pixel (DPP wave_shr:1); "left" and "up-left" stay in registers.  No
//      barrier inside a wave.  Steps come in chunks of PNG_CHUNK = 64; per chunk the wave stages the 64 x 192 filtered bytes it is about to
//      consume into its own LDS tile with coalesced aligned dword loads (16 lanes per row, 12 bytes each; the tile is skewed like the wavefront:
//      tile[l][j] is pixel 64 q + j - l of row l), overwrites them in place with the reconstruction and writes the tile out the same way
//      (16 lanes per row, 12 bytes each: two aligned dwords funnel-shifted to the page row's alignment, the bytes before and after them singly).
//      Rows of a tile are 196 bytes apart (49 dwords, odd: the 64 lanes of a tile access sit on different banks).
//      The step itself has no branch: the lanes of a wave hold rows of different filter types, so the type is four byte masks that select among
//      Sub / Up / Average / Paeth (png_recon); about 90 instructions per step, one dependent chain, so a band costs (W + 63) steps of latency and
//      the launch is as fast as its longest row range -- which is why ldetr_png_scan cuts a page into ranges of about one band wherever a row allows.
//      Bands chain through the last row of the band before, kept in LDS (3 W bytes): band k + 1 runs PNG_LAG = 2 chunks behind band k (lane 63
//      of band k finishes pixel x at step x + 63, so after two chunks the 64 pixels lane 0 of band k + 1 needs are there), waves of the workgroup
//      take bands round-robin, and one __syncthreads per chunk orders the hand-off.  No workgroup ever waits for another one: no flags, no spins.
//      Arithmetic is PNG's: Average = (a + b) >> 1 on the 9-bit sum, Paeth ties resolve a, b, c; zeros above the first row and left of the first pixel.
// Every source index that comes from a device table is clamped to its file (gather) or to the stream buffer (unfilter): a stale device table gives
// wrong pixels, never an access outside the buffers the entry was given.  The entry validates the HOST tables before any launch.
#include <vector>

#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"
#include "png_pages.hpp"

namespace ldetr {

constexpr int PNG_WAVES = 4;
constexpr int PNG_THREADS = PNG_WAVES * 64;
constexpr int PNG_CHUNK = 64;                 // steps (pixels) per chunk
constexpr int PNG_LAG = 2;                    // chunks between consecutive bands
constexpr int PNG_TILE_PITCH = 196;           // bytes per tile row: 3 * PNG_CHUNK + 4
constexpr int PNG_GATHER_THREADS = 256;

// ------------------------------------------------------------------------------------------------------------------------------------------------
// host scan

struct IdatRun { int64_t off, len; };

// The IDAT payloads of a file as one logical byte stream.
struct IdatCursor {
    const uint8_t* file;
    const std::vector<IdatRun>* runs;
    size_t r = 0;
    int64_t i = 0;
    bool skip_empty() {
        while (r < runs->size() && i >= (*runs)[r].len) { r++; i = 0; }
        return r < runs->size();
    }
    bool next(uint8_t* v) {
        if (!skip_empty()) return false;
        *v = file[(*runs)[r].off + i++];
        return true;
    }
    // the longest contiguous piece of at most `want` bytes at the cursor: file offset and length (0 at the end of the stream)
    int64_t piece(int64_t want, int64_t* file_off) {
        if (!skip_empty()) return 0;
        const int64_t n = std::min(want, (*runs)[r].len - i);
        *file_off = (*runs)[r].off + i;
        i += n;
        return n;
    }
};

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_png_scan(const uint8_t* file, int64_t file_bytes, int* width, int* height, int* channels, int64_t* segments, int64_t segments_capacity,
                              int64_t* segments_count, int32_t* row_starts, int64_t row_starts_capacity, int64_t* row_starts_count) {
    LDETR_CHECK(file && file_bytes >= 0 && width && height && channels && segments_count, "png_scan: bad arguments");
    LDETR_CHECK(segments_capacity >= 0 && row_starts_capacity >= 0, "png_scan: negative capacity");
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (file_bytes < 8) PNG_MALFORMED("png_scan: truncated file (%ld bytes, no signature)", (long)file_bytes);
    if (memcmp(file, sig, 8) != 0) PNG_MALFORMED("png_scan: bad signature");
    // chunks
    std::vector<IdatRun> runs;
    int64_t pos = 8;
    bool have_ihdr = false, have_iend = false;
    uint32_t W = 0, H = 0;
    int depth = 0, ctype = 0, interlace = 0;
    while (pos < file_bytes) {
        if (file_bytes - pos < 12) PNG_MALFORMED("png_scan: truncated file (chunk header at byte %ld)", (long)pos);
        const int64_t len = be32(file + pos);
        const uint8_t* type = file + pos + 4;
        if (len > file_bytes - pos - 12) PNG_MALFORMED("png_scan: chunk %.4s at byte %ld: length %ld reaches past the end of the file", (const char*)type, (long)pos, (long)len);
        if (!have_ihdr) {
            if (memcmp(type, "IHDR", 4) != 0 || len != 13) PNG_MALFORMED("png_scan: the first chunk is not a 13-byte IHDR");
            const uint8_t* d = file + pos + 8;
            W = be32(d); H = be32(d + 4); depth = d[8]; ctype = d[9]; interlace = d[12];
            if (W == 0 || H == 0 || W > 0x7fffffffu || H > 0x7fffffffu) PNG_MALFORMED("png_scan: IHDR size %u x %u", W, H);
            if (d[10] != 0 || d[11] != 0 || interlace > 1) PNG_MALFORMED("png_scan: IHDR compression %d / filter %d / interlace %d", d[10], d[11], interlace);
            const bool depth_ok = (ctype == 0 && (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)) || (ctype == 3 && (depth == 1 || depth == 2 || depth == 4 || depth == 8)) ||
                                  ((ctype == 2 || ctype == 4 || ctype == 6) && (depth == 8 || depth == 16));
            if (!depth_ok) PNG_MALFORMED("png_scan: IHDR colour type %d with bit depth %d", ctype, depth);
            have_ihdr = true;
        } else if (memcmp(type, "IDAT", 4) == 0) {
            runs.push_back({pos + 8, len});
        } else if (memcmp(type, "IEND", 4) == 0) {
            have_iend = true;
            break;
        }
        pos += 12 + len;
    }
    if (!have_ihdr) PNG_MALFORMED("png_scan: truncated file (no IHDR)");
    if (!have_iend) PNG_MALFORMED("png_scan: no IEND chunk");
    *width = (int)W; *height = (int)H;
    *channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4;
    if (interlace) PNG_NOT_ELIGIBLE("png_scan: interlaced");
    if (ctype == 3) PNG_NOT_ELIGIBLE("png_scan: palette image");
    if (depth != 8) PNG_NOT_ELIGIBLE("png_scan: %d-bit samples", depth);
    if (ctype != 2) PNG_NOT_ELIGIBLE("png_scan: colour type %d (grey, grey-alpha or RGBA); the device path takes 8-bit RGB", ctype);
    if (W > (uint32_t)PNG_MAX_W || H > (uint32_t)PNG_MAX_H) PNG_NOT_ELIGIBLE("png_scan: %u x %u is larger than the device path takes (%d x %d)", W, H, PNG_MAX_W, PNG_MAX_H);
    // zlib stream
    const int64_t stride = 1 + 3 * (int64_t)W, total = stride * (int64_t)H;
    IdatCursor cur{file, &runs};
    uint8_t cmf, flg;
    if (!cur.next(&cmf) || !cur.next(&flg)) PNG_MALFORMED("png_scan: truncated zlib stream (no header)");
    if ((cmf & 0x0f) != 8 || (cmf >> 4) > 7 || (((unsigned)cmf << 8) | flg) % 31 != 0) PNG_MALFORMED("png_scan: bad zlib header %02x %02x", cmf, flg);
    if (flg & 0x20) PNG_NOT_ELIGIBLE("png_scan: zlib stream with a preset dictionary");
    int64_t nseg = 0, nrow = 0, done = 0, last_start = 0, next_row = 0;      // next_row: the first row whose filter byte has not been seen yet
    bool final_block = false;
    while (!final_block) {
        uint8_t hdr, l0, l1, n0, n1;
        if (!cur.next(&hdr)) PNG_MALFORMED("png_scan: truncated zlib stream (no final block after %ld payload bytes)", (long)done);
        final_block = hdr & 1;
        const int btype = (hdr >> 1) & 3;
        if (btype == 3) PNG_MALFORMED("png_scan: deflate block of reserved type 3");
        if (btype != 0) PNG_NOT_ELIGIBLE("png_scan: compressed deflate block (type %d); the device path takes stored blocks only", btype);
        if (!cur.next(&l0) || !cur.next(&l1) || !cur.next(&n0) || !cur.next(&n1)) PNG_MALFORMED("png_scan: truncated zlib stream (stored-block header)");
        const unsigned blen = l0 | ((unsigned)l1 << 8), nlen = n0 | ((unsigned)n1 << 8);
        if ((blen ^ nlen) != 0xffffu) PNG_MALFORMED("png_scan: stored block with LEN %04x, NLEN %04x (not its complement)", blen, nlen);
        int64_t left = blen;
        if (done + left > total) PNG_MALFORMED("png_scan: more than the %ld payload bytes of a %u x %u RGB page", (long)total, W, H);
        while (left > 0) {
            int64_t fo = 0;
            const int64_t n = cur.piece(left, &fo);
            if (n == 0) PNG_MALFORMED("png_scan: truncated zlib stream (stored block reaches past the last IDAT chunk)");
            for (; next_row * stride < done + n; next_row++) {           // the filter bytes inside this piece
                const uint8_t fb = file[fo + next_row * stride - done];
                if (fb > 4) PNG_MALFORMED("png_scan: row %ld has filter byte %d", (long)next_row, fb);
                if (next_row == 0 || (fb <= 1 && next_row - last_start >= PNG_MIN_RANGE)) {
                    if (row_starts && nrow < row_starts_capacity) row_starts[nrow] = (int32_t)next_row;
                    nrow++;
                    last_start = next_row;
                }
            }
            if (segments && nseg < segments_capacity) { segments[3 * nseg] = fo; segments[3 * nseg + 1] = done; segments[3 * nseg + 2] = n; }
            nseg++;
            done += n; left -= n;
        }
    }
    if (done != total) PNG_MALFORMED("png_scan: %ld payload bytes, a %u x %u RGB page has %ld", (long)done, W, H, (long)total);
    for (int k = 0; k < 4; k++) {
        uint8_t v;
        if (!cur.next(&v)) PNG_MALFORMED("png_scan: truncated zlib stream (no Adler-32)");
    }
    *segments_count = nseg;
    if (row_starts_count) *row_starts_count = nrow;
    LDETR_CHECK(!segments || nseg <= segments_capacity, "png_scan: segment table too small (%ld entries, %ld needed)", (long)segments_capacity, (long)nseg);
    LDETR_CHECK(!row_starts || nrow <= row_starts_capacity, "png_scan: row-start table too small (%ld entries, %ld needed)", (long)row_starts_capacity, (long)nrow);
    return LDETR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// device

namespace ldetr {

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (a) one payload run per block iteration
__global__ void __launch_bounds__(PNG_GATHER_THREADS) png_gather_kernel(PngParams p) {
    const long S = (long)p.H * (1 + 3L * p.W);
    for (long s = blockIdx.x; s < p.k; s += gridDim.x) {
        const int64_t* q = p.seg + 4 * s;
        const long img = q[0], so = q[1], doff = q[2], len = q[3];
        if (img < 0 || img >= p.n || len <= 0 || doff < 0 || doff > S - len) continue;              // a stale table: nothing leaves the stream buffer
        const long f0 = clampl(p.file_off[img], 0, p.files_bytes), f1 = clampl(p.file_off[img + 1], f0, p.files_bytes);
        if (f1 <= f0) continue;
        const long src0 = f0 + so;                                                                   // absolute byte offsets; every read index is clamped to [f0, f1)
        const long dst0 = img * S + doff;
        const long w_lo = f0 >> 2, w_hi = (f1 - 1) >> 2;                                            // the aligned dwords that hold bytes of this file
        const uint32_t* fw = reinterpret_cast<const uint32_t*>(p.files);
        const long head = min(len, (4 - (dst0 & 3)) & 3);
        const long body = (len - head) >> 2;                                                        // destination dwords
        const long tail0 = head + 4 * body;
        for (long i = threadIdx.x; i < head + (len - tail0); i += PNG_GATHER_THREADS) {             // bytes at the two ends
            const long b = i < head ? i : tail0 + (i - head);
            p.stream[dst0 + b] = p.files[clampl(src0 + b, f0, f1 - 1)];
        }
        const long sb = src0 + head, db = dst0 + head;                                               // db is a multiple of 4
        if (((sb ^ db) & 15) == 0 && sb >= f0 && sb + 4 * body <= f1) {
            // source and destination agree modulo 16: dwords up to a 16-byte boundary, then 16-byte vectors
            const long pre = min(body, ((16 - (db & 15)) & 15) >> 2), vec = (body - pre) >> 2, post0 = pre + 4 * vec;
            uint32_t* dw = reinterpret_cast<uint32_t*>(p.stream + db);
            const uint32_t* sw = reinterpret_cast<const uint32_t*>(p.files + sb);
            for (long i = threadIdx.x; i < pre + (body - post0); i += PNG_GATHER_THREADS) {
                const long d = i < pre ? i : post0 + (i - pre);
                dw[d] = sw[d];
            }
            uint4* dv = reinterpret_cast<uint4*>(dw + pre);
            const uint4* sv = reinterpret_cast<const uint4*>(sw + pre);
            for (long i = threadIdx.x; i < vec; i += PNG_GATHER_THREADS) dv[i] = sv[i];
        } else {
            const unsigned sh = (unsigned)(sb & 3);
            const long w0 = sb >> 2;                                                                 // floor: sb may be negative only for a stale table (clamped below)
            uint32_t* dw = reinterpret_cast<uint32_t*>(p.stream + db);
            for (long i = threadIdx.x; i < body; i += PNG_GATHER_THREADS) {
                const uint32_t lo = fw[clampl(w0 + i, w_lo, w_hi)], hi = fw[clampl(w0 + i + 1, w_lo, w_hi)];
                dw[i] = __builtin_amdgcn_alignbyte(hi, lo, sh);
            }
        }
    }
}

__device__ __forceinline__ unsigned png_wave_shr1(unsigned v) {
    // lane l receives lane l - 1's value (lane 0 keeps its own)
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
}

// One pixel, three channels packed in the low 24 bits, no branch (the lanes of a wave hold rows of different filter types): the row's filter type
// is four byte masks m1 .. m4 (the one that is set selects Sub / Up / Average / Paeth; none set = None), the predictor is
// (a & m1) | (b & m2) | (avg & m3) | (paeth & m4).  Average and the final sum are per-byte SWAR (no carry crosses a byte); Paeth is per channel.
__device__ __forceinline__ unsigned png_recon(unsigned f, unsigned a, unsigned b, unsigned c, unsigned m1, unsigned m2, unsigned m3, unsigned m4) {
    const unsigned avg = (a & b) + (((a ^ b) & 0xfefefeu) >> 1);                 // floor((a + b) / 2) per byte: the 9-bit sum, halved
    unsigned paeth = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const int fa = (int)__builtin_amdgcn_ubfe(a, 8 * ch, 8), fb = (int)__builtin_amdgcn_ubfe(b, 8 * ch, 8), fc = (int)__builtin_amdgcn_ubfe(c, 8 * ch, 8);
        const int dbc = fb - fc, dac = fa - fc, dsum = dbc + dac;
        const int pa = max(dbc, -dbc), pb = max(dac, -dac), pc = max(dsum, -dsum);
        const int inner = pb <= pc ? fb : fc;
        const int p = pa <= min(pb, pc) ? fa : inner;                            // ties: a, then b, then c
        paeth |= (unsigned)p << (8 * ch);
    }
    const unsigned pred = (a & m1) | (b & m2) | (avg & m3) | (paeth & m4);
    return (((f & 0x7f7f7fu) + (pred & 0x7f7f7fu)) ^ ((f ^ pred) & 0x808080u)) & 0xffffffu;      // per-byte sum modulo 256
}

// (b) one workgroup per (page, independent row range)
__global__ void __launch_bounds__(PNG_THREADS) png_unfilter_kernel(PngParams p) {
    __shared__ uint32_t tiles[PNG_WAVES][64 * PNG_TILE_PITCH / 4];
    __shared__ uint8_t uprow[3 * PNG_MAX_W];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int img = p.jobs[3 * blockIdx.x], row0 = p.jobs[3 * blockIdx.x + 1], row1 = p.jobs[3 * blockIdx.x + 2];
    if (img < 0 || img >= p.n || row0 < 0 || row1 > p.H || row1 <= row0) return;                     // uniform per block (a stale table)
    const int W = p.W;
    const long stride = 1 + 3L * W;
    const int K = (row1 - row0 + 63) >> 6;                                                           // bands
    const int Q = (W + 63 + PNG_CHUNK - 1) / PNG_CHUNK;                                              // chunks per band: steps 0 .. W + 62
    const int R = max(Q, PNG_WAVES * PNG_LAG);                                                       // band k starts at phase (k / PNG_WAVES) * R + (k % PNG_WAVES) * PNG_LAG
    const int P = ((K - 1) / PNG_WAVES) * R + ((K - 1) % PNG_WAVES) * PNG_LAG + Q;
    uint32_t* tile = tiles[wave];
    uint8_t* tile_b = reinterpret_cast<uint8_t*>(tile);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(p.stream);
    const long sw_hi = (p.stream_bytes >> 2) - 1;
    unsigned left = 0, upleft = 0, prev = 0;
    unsigned m1 = 0, m2 = 0, m3 = 0, m4 = 0;                                                         // the row's filter type as byte masks (png_recon)
    for (int ph = 0; ph < P; ph++) {
        const int t = ph - wave * PNG_LAG;
        const int g = t >= 0 ? t / R : 0, q = t >= 0 ? t - g * R : 0;
        const int band = g * PNG_WAVES + wave;
        if (t >= 0 && band < K && q < Q) {                                                           // uniform per wave
            const int y0 = row0 + band * 64;
            const int y = y0 + lane;
            const bool row_ok = y < row1;
            const int yc = row_ok ? y : row1 - 1;
            if (q == 0) {
                left = upleft = prev = 0;
                const int ft = p.stream[clampl(((long)img * p.H + yc) * stride, 0, p.stream_bytes - 1)];
                m1 = ft == 1 ? 0xffffffu : 0u; m2 = ft == 2 ? 0xffffffu : 0u; m3 = ft == 3 ? 0xffffffu : 0u; m4 = ft == 4 ? 0xffffffu : 0u;
            }
            // stage in: tile[r][i] = filtered byte 1 + 3 (64 q - r) + i of row r, 16 lanes x 12 bytes per row, four rows per pass
            {
                const int sub = lane >> 4, l16 = lane & 15;
#pragma unroll 4
                for (int r4 = 0; r4 < 64; r4 += 4) {
                    const int r = r4 + sub;
                    const int yr = min(y0 + r, row1 - 1);
                    const long A = ((long)img * p.H + yr) * stride + 1 + 3L * (PNG_CHUNK * q - r) + 12 * l16;
                    const long w0 = A >> 2;
                    const unsigned sh = (unsigned)(A & 3);
                    const uint32_t d0 = sw[clampl(w0, 0, sw_hi)], d1 = sw[clampl(w0 + 1, 0, sw_hi)], d2 = sw[clampl(w0 + 2, 0, sw_hi)], d3 = sw[clampl(w0 + 3, 0, sw_hi)];
                    uint32_t* t3 = tile + r * (PNG_TILE_PITCH / 4) + 3 * l16;
                    t3[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
                    t3[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
                    t3[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
                }
            }
            // the row above lane 0: 64 pixels of the band before, one per lane
            unsigned upreg = 0;
            if (band > 0) {
                const int x = min(PNG_CHUNK * q + lane, W - 1);
                upreg = uprow[3 * x] | ((unsigned)uprow[3 * x + 1] << 8) | ((unsigned)uprow[3 * x + 2] << 16);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t* mine = tile + lane * (PNG_TILE_PITCH / 4);
            const int xbase = PNG_CHUNK * q - lane;
#pragma unroll 1
            for (int j4 = 0; j4 < PNG_CHUNK; j4 += 4) {
                const uint32_t w0 = mine[3 * (j4 >> 2)], w1 = mine[3 * (j4 >> 2) + 1], w2 = mine[3 * (j4 >> 2) + 2];
                unsigned f[4] = {w0 & 0xffffffu, (w0 >> 24) | ((w1 & 0xffffu) << 8), (w1 >> 16) | ((w2 & 0xffu) << 16), w2 >> 8};
                unsigned o[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int x = xbase + j4 + u;
                    unsigned up = png_wave_shr1(prev);
                    const unsigned up0 = (unsigned)__builtin_amdgcn_readlane((int)upreg, j4 + u);
                    if (lane == 0) up = up0;
                    const bool valid = row_ok && x >= 0 && x < W;
                    const unsigned out = png_recon(f[u], left, up, upleft, m1, m2, m3, m4);
                    o[u] = out;
                    if (valid) { left = out; upleft = up; prev = out; }
                }
                mine[3 * (j4 >> 2)] = o[0] | (o[1] << 24);
                mine[3 * (j4 >> 2) + 1] = (o[1] >> 8) | (o[2] << 16);
                mine[3 * (j4 >> 2) + 2] = (o[2] >> 16) | (o[3] << 8);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // store out: row r's bytes [3 (64 q - r), + 192) of the page row, cut to [0, 3 W)
            {
                const int sub = lane >> 4, l16 = lane & 15;
#pragma unroll 1
                for (int r4 = 0; r4 < 64; r4 += 4) {
                    const int r = r4 + sub;
                    if (y0 + r >= row1) continue;
                    const long b0 = 3L * (PNG_CHUNK * q - r) + 12 * l16;                             // byte offset in the page row
                    uint8_t* drow = p.dst + ((long)img * p.H + y0 + r) * 3L * W;
                    const uint32_t* t3 = tile + r * (PNG_TILE_PITCH / 4) + 3 * l16;
                    if (b0 >= 0 && b0 + 12 <= 3L * W) {
                        // all 12 bytes inside the row: the bytes up to the next aligned address, two aligned dwords (funnel-shifted), the bytes after them
                        const uint32_t t0 = t3[0], t1 = t3[1], t2 = t3[2];
                        const unsigned mis = (unsigned)((uintptr_t)(drow + b0) & 3), head = (4 - mis) & 3;
                        uint32_t* d = reinterpret_cast<uint32_t*>(drow + b0 + head);
                        d[0] = __builtin_amdgcn_alignbyte(t1, t0, head);
                        d[1] = __builtin_amdgcn_alignbyte(t2, t1, head);
                        if (mis == 0) {
                            d[2] = t2;
                        } else {
#pragma unroll
                            for (unsigned i = 0; i < 3; i++) {
                                if (i < head) drow[b0 + i] = (uint8_t)(t0 >> (8 * i));
                                if (i < mis) drow[b0 + 12 - mis + i] = (uint8_t)(t2 >> (8 * (4 - mis + i)));
                            }
                        }
                    } else {
                        const uint8_t* tb = reinterpret_cast<const uint8_t*>(t3);
                        for (int i = 0; i < 12; i++)
                            if (b0 + i >= 0 && b0 + i < 3L * W) drow[b0 + i] = tb[i];
                    }
                }
            }
            // hand the band's last row to the band after it: pixels 64 q + j - 63 of tile row 63
            if (band + 1 < K) {
                const int x = PNG_CHUNK * q + lane - 63;
                if (x >= 0 && x < W) {
                    const uint8_t* tb = tile_b + 63 * PNG_TILE_PITCH + 3 * lane;
                    uprow[3 * x] = tb[0]; uprow[3 * x + 1] = tb[1]; uprow[3 * x + 2] = tb[2];
                }
            }
        }
        __syncthreads();
    }
}

// what ldetr_png_decode_u8 and ldetr_png_inflate_u8 (png_inflate.hip) share: the checks of the host tables both take, and the unfilter launch
int png_check_file_offsets(const char* who, int n, const int64_t* file_off, int64_t files_bytes) {
    for (int i = 0; i <= n; i++) {
        const int64_t o = file_off[i];
        LDETR_CHECK(o >= 0 && o <= files_bytes && (i == 0 || o >= file_off[i - 1]), "%s: file offset table: entry %d = %ld", who, i, (long)o);
    }
    return LDETR_OK;
}

// the row ranges of a page tile [0, H) in order
int png_check_jobs(const char* who, int n, int H, const int32_t* jobs, int64_t n_jobs) {
    int64_t page = 0, run = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const int32_t* q = jobs + 3 * j;
        if (q[0] != page) {
            LDETR_CHECK(q[0] == page + 1 && run == H, "%s: the row ranges of page %ld do not tile its %d rows", who, (long)page, H);
            page = q[0]; run = 0;
        }
        LDETR_CHECK(q[0] < n && q[1] == run && q[2] > q[1] && q[2] <= H, "%s: row range %ld = (%d, %d, %d) does not continue page %ld at row %ld", who, (long)j, q[0], q[1], q[2], (long)page, (long)run);
        run = q[2];
    }
    LDETR_CHECK(page == n - 1 && run == H, "%s: the row ranges of page %ld do not tile its %d rows", who, (long)page, H);
    return LDETR_OK;
}

int png_launch_unfilter(const PngParams& p, int64_t n_jobs, hipStream_t st, const char* what) {
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n_jobs), PNG_THREADS, 0, st, p);
    return check_launch(what);
}

}  // namespace ldetr

extern "C" int ldetr_png_decode_u8(const ldetr_png_decode_args* a, void* stream) {
    LDETR_CHECK_BLOCK(a, ldetr_png_decode_args, "png_decode");
    const int n = a->n, H = a->H, W = a->W;
    LDETR_CHECK(n >= 0 && n <= 65535, "png_decode: 0 <= pages <= 65535 (got %d)", n);
    if (n == 0) return LDETR_OK;
    LDETR_CHECK(W >= 1 && W <= PNG_MAX_W && H >= 1 && H <= PNG_MAX_H, "png_decode: page %d x %d outside [1, %d] x [1, %d]", W, H, PNG_MAX_W, PNG_MAX_H);
    LDETR_CHECK((a->phases & ~3) == 0 && a->phases != 0, "png_decode: phases %d (1 gather, 2 unfilter, 3 both)", a->phases);
    LDETR_CHECK(a->files && a->file_off && a->file_off_dev && a->segments && a->segments_dev && a->jobs && a->jobs_dev && a->scratch && a->dst, "png_decode: null pointer");
    LDETR_CHECK(a->files_bytes > 0 && a->files_bytes % 16 == 0 && ((uintptr_t)a->files & 15) == 0, "png_decode: the file buffer must be 16-byte aligned and a multiple of 16 bytes long");
    const int64_t stride = 1 + 3 * (int64_t)W, S = stride * H;
    const int64_t need = (n * S + 15) / 16 * 16;
    LDETR_CHECK(((uintptr_t)a->scratch & 15) == 0 && a->scratch_bytes % 16 == 0 && a->scratch_bytes >= need, "png_decode: scratch must be 16-byte aligned and hold %ld bytes (a multiple of 16; got %ld)",
                (long)need, (long)a->scratch_bytes);
    LDETR_CHECK(((uintptr_t)a->dst & 3) == 0, "png_decode: dst must be 4-byte aligned");
    LDETR_CHECK(a->n_segments >= 1 && a->n_jobs >= n && a->n_jobs <= (int64_t)n * PNG_MAX_H, "png_decode: %ld segments, %ld row ranges for %d pages", (long)a->n_segments, (long)a->n_jobs, n);
    int rc = png_check_file_offsets("png_decode", n, a->file_off, a->files_bytes);
    if (rc) return rc;
    // every segment inside its file; the stream offsets of a page tile [0, S) in order
    int64_t page = 0, run = 0;
    for (int64_t s = 0; s < a->n_segments; s++) {
        const int64_t* q = a->segments + 4 * s;
        LDETR_CHECK(q[0] >= 0 && q[0] < n, "png_decode: segment %ld names page %ld of %d", (long)s, (long)q[0], n);
        if (q[0] != page) {
            LDETR_CHECK(q[0] == page + 1 && run == S, "png_decode: the segments of page %ld do not tile its %ld stream bytes (they end at %ld)", (long)page, (long)S, (long)run);
            page = q[0]; run = 0;
        }
        const int64_t flen = a->file_off[q[0] + 1] - a->file_off[q[0]];
        LDETR_CHECK(q[3] >= 0 && q[1] >= 0 && q[1] <= flen && q[3] <= flen - q[1], "png_decode: segment %ld (offset %ld, length %ld) leaves its file of %ld bytes", (long)s, (long)q[1], (long)q[3], (long)flen);
        LDETR_CHECK(q[2] == run && q[3] <= S - run, "png_decode: segment %ld does not continue the stream of page %ld (offset %ld, expected %ld, length %ld of %ld)", (long)s, (long)page, (long)q[2],
                    (long)run, (long)q[3], (long)S);
        run += q[3];
    }
    LDETR_CHECK(page == n - 1 && run == S, "png_decode: the segments of page %ld do not tile its %ld stream bytes (they end at %ld)", (long)page, (long)S, (long)run);
    rc = png_check_jobs("png_decode", n, H, a->jobs, a->n_jobs);
    if (rc) return rc;
    PngParams p;
    p.files = a->files; p.files_bytes = a->files_bytes; p.file_off = a->file_off_dev; p.seg = a->segments_dev; p.k = a->n_segments; p.jobs = a->jobs_dev;
    p.stream = a->scratch; p.stream_bytes = a->scratch_bytes; p.dst = a->dst; p.n = n; p.H = H; p.W = W;
    hipStream_t st = (hipStream_t)stream;
    if (a->phases & 1) {
        hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)std::min<int64_t>(a->n_segments, 8192)), PNG_GATHER_THREADS, 0, st, p);
        rc = check_launch("png_decode (gather)");
        if (rc) return rc;
    }
    if (a->phases & 2) {
        return png_launch_unfilter(p, a->n_jobs, st, "png_decode (unfilter)");
    }
    return LDETR_OK;
}
