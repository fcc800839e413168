// A uint8 [H][W][3] grid in GPU memory encoded as a PNG file on the device: row filters, deflate, chunk framing and every checksum.
// The host receives the finished file bytes: it never reads pixels, filtered rows or a payload.  Three launches, ordered by launch boundaries only:
//  (a) png_enc_filter_kernel: one workgroup per row.  The five PNG filter types are scored by the sum of absolute residuals (residuals read as signed
//      bytes, ties to the lowest type), the winner's residuals go to the filtered scanline stream [H][1 + 3 W] in the workspace.
//  (b) png_enc_deflate_kernel: one workgroup per segment of PE_SEG = 64 KiB of that stream, held in LDS.  No back-reference crosses a segment start.
//      The segment is cut into sub-blocks of PE_SUB = 512 bytes, one lane parses one sub-block greedily: at every position the candidate distances
//      {1, 2, 3, 4, 6, 9, 12, row - 3, row, row + 3, 2 row} (row = 1 + 3 W, each at most 32768) are tried, the longest match of 3 .. 258 bytes that ends
//      inside the sub-block wins; there is no hash table.  Tokens stay in LDS (one byte array beside the data: 0 = literal, else candidate + 1 followed
//      by length - 3).  The token histogram gives the dynamic Huffman code (leaves ranked in parallel, the two-queue merge by one lane, frequencies
//      halved and the tree rebuilt while a code is longer than 15 bits), then the three block sizes -- stored, fixed, dynamic -- exactly, before any bit
//      is written; the smallest wins (ties to the lower type), so a segment never outgrows its stored form.  Bit offsets of the sub-blocks come from a
//      scan of their bit counts.  A byte of the output is written by the one lane whose bits contain the byte's first bit: that lane keeps walking the
//      tokens of the following sub-blocks (all in LDS) until its last byte is full.  No atomics on output bytes, no read-modify-write.
//      A compressed segment ends with an empty stored block (pad to the byte, 00 00 FF FF), so the next one starts byte-aligned; the last segment's
//      is the final block.  A stored segment is byte-aligned as it is.  The dynamic header is HCLEN = 19 with a flat code-length code (symbols 0 .. 15
//      get 4 bits, 16 .. 18 none): every code length follows as 4 bits.  Fewer than two distance codes in use: two codes of length 1 are sent.
//      The segment's deflate bytes go to a slot of the workspace; its size, block type and Adler-32 partial sums to a row of the segment table.
//  (c) png_enc_assemble_kernel: one workgroup per segment = one IDAT chunk.  Its place in the file is the sum of the chunk sizes before it (every
//      workgroup adds them up for itself), the payload is copied there and its CRC-32 computed from per-lane slices joined with zlib's crc32_combine
//      arithmetic (x^(8 n) modulo the CRC polynomial).  The first workgroup writes the signature and IHDR, the last one joins the Adler-32 partial
//      sums, appends the Adler-32 to its chunk, writes IEND and the total length.
// With an index requested (bit 0 of ldetr_png_encode_args.reserved) the file carries one more chunk, ldIX, in front of the first IDAT:
// (a) writes the filter type of every row and (b) the bit offset of every sub-block's first token (what its scan computes anyway) into the chunk's payload in the
// workspace, and (c) runs one more workgroup that frames it like a segment's chunk while the others start that much later in the file.  Without the bit
// not one byte of the file changes.
// The kernels are written as phases of "every thread does this" separated by workgroup barriers (PNG_EACH_THREAD); the same source runs a phase as a
// loop over the thread index when compiled for the host, which is how the encoder is checked against zlib without a GPU.
// Every size the assemble kernel reads from the segment table is clamped to the slot and to the output buffer before it is used.
#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"

namespace ldetr {

constexpr int PE_SEG = 65536;                 // bytes of filtered stream per segment (mirrored by render.PNG_ENCODE_SEGMENT)
constexpr int PE_SUB = 512;                   // bytes per sub-block: one lane's parse; longer than the longest match (258)
constexpr int PE_NSUB = PE_SEG / PE_SUB;
constexpr int PE_THREADS = 128;               // deflate kernel: one lane per sub-block
constexpr int PE_FILTER_THREADS = 256;
constexpr int PE_ASM_THREADS = 256;
constexpr int PE_SLICE = 260;                 // bytes per lane of a CRC piece: 65 dwords, an odd stride
constexpr int PE_PIECE = PE_ASM_THREADS * PE_SLICE;
constexpr long PE_SLOT = 2L * PE_SEG + 512;   // bytes of workspace per segment: a forced dynamic block is at most 16 bits per byte + header + trailer
constexpr int PE_META = 8;                    // int64 per row of the workspace's segment table
constexpr int PE_MAXC = 12;                   // candidate distances
constexpr int PE_MAX_DIM = 16384;
constexpr int PE_DBASE = 288;                 // distance symbols sit behind the 288 literal / length symbols in the code tables
constexpr int PE_NSYM = 320;
constexpr unsigned PE_ADLER = 65521u;
constexpr long PE_FILE_HEAD = 33;             // signature + IHDR chunk

#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_EACH_THREAD(tid, nt) __syncthreads(); for (int tid = threadIdx.x, once_ = 1; once_; once_ = 0)
#define PNG_SYNC() __syncthreads()
#define PNG_ATOMIC_ADD(ptr, v) atomicAdd((ptr), (v))
#else
#define PNG_EACH_THREAD(tid, nt) for (int tid = 0; tid < (nt); tid++)
#define PNG_SYNC() do {} while (0)
#define PNG_ATOMIC_ADD(ptr, v) (*(ptr) += (v))
#endif
#define PNG_HD __host__ __device__ __forceinline__

struct PngEncParams {
    const uint8_t* src;
    int H, W;
    int mode;                                 // 0 auto, 1 stored, 2 fixed, 3 dynamic
    int filter;                               // -1 auto, 0 .. 4 forced
    uint8_t* stream;                          // workspace: [H][1 + 3 W]
    int64_t* meta;                            // workspace: [nseg][PE_META] = (first byte, end byte, block type, chunk bytes, adler a, adler b, 0, 0)
    uint8_t* slots;                           // workspace: [nseg][PE_SLOT]
    long nseg;
    long total;                               // H * (1 + 3 W)
    uint8_t* out; long out_cap;
    int64_t* out_total;
    int64_t* user_table;                      // optional [nseg][4]
    int ncand;
    int cand[PE_MAXC];                        // ascending
    uint8_t* index;                           // workspace, or null: the payload of the ldIX chunk (version, PE_SEG, PE_SUB | filter type [H] | bit offsets, big-endian)
    long index_bytes;                         // its length; the chunk takes 12 more bytes of the file, in front of the first IDAT
};

PNG_HD long png_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }
PNG_HD void png_index_be32(const PngEncParams& p, long at, unsigned v) {
    if (at < 0 || at + 4 > p.index_bytes) return;
    p.index[at] = (uint8_t)(v >> 24); p.index[at + 1] = (uint8_t)(v >> 16); p.index[at + 2] = (uint8_t)(v >> 8); p.index[at + 3] = (uint8_t)v;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// (a) filters.  Arithmetic as png_recon of png_decode.hip undoes it.

PNG_HD unsigned png_residual(int t, int x, int a, int b, int c) {
    int pred = 0;
    if (t == 1) pred = a;
    else if (t == 2) pred = b;
    else if (t == 3) pred = (a + b) >> 1;
    else if (t == 4) {
        const int dbc = b - c, dac = a - c, ds = dbc + dac;
        const int pa = dbc < 0 ? -dbc : dbc, pb = dac < 0 ? -dac : dac, pc = ds < 0 ? -ds : ds;
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (unsigned)(x - pred) & 255u;
}
PNG_HD unsigned png_absres(unsigned r) { return r < 128u ? r : 256u - r; }

struct PngFilterShared { unsigned sum[5]; };

__host__ __device__ inline void png_filter_row(PngFilterShared& S, const PngEncParams& p, long y) {
    const long n = 3L * p.W;
    const uint8_t* cur = p.src + y * n;
    const uint8_t* up = y > 0 ? cur - n : nullptr;
    uint8_t* dst = p.stream + y * (n + 1);
    PNG_EACH_THREAD(tid, PE_FILTER_THREADS) { if (tid < 5) S.sum[tid] = 0u; }
    if (p.filter < 0) {
        PNG_EACH_THREAD(tid, PE_FILTER_THREADS) {
            unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
            for (long i = tid; i < n; i += PE_FILTER_THREADS) {
                const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = up ? up[i] : 0, c = (up && i >= 3) ? up[i - 3] : 0;
                s0 += png_absres(png_residual(0, x, a, b, c)); s1 += png_absres(png_residual(1, x, a, b, c)); s2 += png_absres(png_residual(2, x, a, b, c));
                s3 += png_absres(png_residual(3, x, a, b, c)); s4 += png_absres(png_residual(4, x, a, b, c));
            }
            PNG_ATOMIC_ADD(&S.sum[0], s0); PNG_ATOMIC_ADD(&S.sum[1], s1); PNG_ATOMIC_ADD(&S.sum[2], s2); PNG_ATOMIC_ADD(&S.sum[3], s3); PNG_ATOMIC_ADD(&S.sum[4], s4);
        }
    }
    PNG_EACH_THREAD(tid, PE_FILTER_THREADS) {
        int t = p.filter;
        if (t < 0) {
            t = 0;
            unsigned best = S.sum[0];
            if (S.sum[1] < best) { best = S.sum[1]; t = 1; }
            if (S.sum[2] < best) { best = S.sum[2]; t = 2; }
            if (S.sum[3] < best) { best = S.sum[3]; t = 3; }
            if (S.sum[4] < best) { best = S.sum[4]; t = 4; }
        }
        if (tid == 0) dst[0] = (uint8_t)t;
        if (tid == 0 && p.index) {
            if (12 + y < p.index_bytes) p.index[12 + y] = (uint8_t)t;
            if (y == 0) { png_index_be32(p, 0, 1u); png_index_be32(p, 4, (unsigned)PE_SEG); png_index_be32(p, 8, (unsigned)PE_SUB); }
        }
        for (long i = tid; i < n; i += PE_FILTER_THREADS) {
            const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = up ? up[i] : 0, c = (up && i >= 3) ? up[i - 3] : 0;
            dst[1 + i] = (uint8_t)png_residual(t, x, a, b, c);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// (b) deflate of one segment

PNG_HD int png_log2(unsigned v) { return 31 - __builtin_clz(v); }
// length 3 .. 258 -> symbol 257 .. 285, number of extra bits, their value
PNG_HD void png_len_code(int len, int& sym, int& ebits, int& eval) {
    const int l = len - 3;
    if (len == 258) { sym = 285; ebits = 0; eval = 0; return; }
    if (l < 8) { sym = 257 + l; ebits = 0; eval = 0; return; }
    const int e = png_log2((unsigned)l) - 2;
    sym = 257 + 4 * e + (l >> e); ebits = e; eval = l & ((1 << e) - 1);
}
// distance 1 .. 32768 -> symbol 0 .. 29, number of extra bits, their value
PNG_HD void png_dist_code(int dist, int& sym, int& ebits, int& eval) {
    const int d = dist - 1;
    if (d < 4) { sym = d; ebits = 0; eval = 0; return; }
    const int e = png_log2((unsigned)d) - 1;
    sym = 2 * e + (d >> e); ebits = e; eval = d & ((1 << e) - 1);
}
PNG_HD int png_sym_extra(int s) {            // extra bits of a symbol of the joint table
    if (s < PE_DBASE) return (s < 265 || s >= 285) ? 0 : (s - 261) >> 2;
    const int d = s - PE_DBASE;
    return d < 4 ? 0 : (d >> 1) - 1;
}
PNG_HD int png_fixed_len(int s) { return s >= PE_DBASE ? 5 : (s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8))); }
PNG_HD unsigned png_rev(unsigned code, int len) {
    unsigned r = 0;
    for (int i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}
PNG_HD long png_stored_bytes(long n) { return n + 5 * ((n + 65534) / 65535); }

struct PngDeflateShared {
    uint8_t data[PE_SEG];
    uint8_t tok[PE_SEG];
    unsigned freq[PE_NSYM];                   // token histogram
    unsigned wfreq[PE_NSYM];                  // what the tree is built from: + the dummy distance codes, halved while the code is too long
    unsigned short code[PE_NSYM];             // bit-reversed: ready to be put LSB first
    uint8_t clen[PE_NSYM];
    unsigned short sorted[PE_NSYM];           // used symbols by (frequency, index): literal / length tree at 0, distance tree at PE_DBASE
    unsigned nfreq[2 * PE_NSYM];              // tree nodes: leaves then internal nodes; literal / length tree at 0, distance tree at 2 * PE_DBASE
    unsigned short parent[2 * PE_NSYM];
    uint8_t depth[2 * PE_NSYM];
    unsigned blc[16], nextc[16];
    unsigned bits[PE_NSUB];
    unsigned off[PE_NSUB + 1];
    int cand[PE_MAXC];
    unsigned adler_a;
    unsigned long long adler_b;
    int over, type, hlit, hdist;
    unsigned hdr_bits, total_bits;
};

struct PngBitWriter {
    uint8_t* base;                            // the segment's deflate bytes
    long cap;
    long pos;                                 // next byte
    long skip;                                // a first byte that another lane owns (-1: none)
    long lim;                                 // bytes at or past it are not this lane's
    unsigned long long acc;
    int n;
    PNG_HD void put(unsigned v, int len) {
        acc |= (unsigned long long)v << n;
        n += len;
        while (n >= 8) {
            if (pos != skip && pos < lim && pos < cap) base[pos] = (uint8_t)(acc & 0xffu);
            pos++; acc >>= 8; n -= 8;
        }
    }
};

// the token at position i of the segment (i == n: the end-of-block code and the empty stored block's header, padded to the byte); returns the next position
PNG_HD int png_put_token(PngDeflateShared& S, PngBitWriter& w, int i, int n, bool last_seg) {
    if (i >= n) {
        w.put(S.code[256], S.clen[256]);
        w.put(last_seg ? 1u : 0u, 1); w.put(0u, 2);
        if (w.n & 7) w.put(0u, 8 - (w.n & 7));
        return n + 1;
    }
    const int t = S.tok[i];
    if (t == 0) {
        const int b = S.data[i];
        w.put(S.code[b], S.clen[b]);
        return i + 1;
    }
    const int len = (int)S.tok[i + 1] + 3;
    int sym, eb, ev;
    png_len_code(len, sym, eb, ev);
    w.put(S.code[sym], S.clen[sym]);
    if (eb) w.put((unsigned)ev, eb);
    png_dist_code(S.cand[(t - 1) % PE_MAXC], sym, eb, ev);
    w.put(S.code[PE_DBASE + sym], S.clen[PE_DBASE + sym]);
    if (eb) w.put((unsigned)ev, eb);
    return i + len;
}

// one lane: Huffman code lengths of one tree from its ranked leaves; false if a code is longer than 15 bits
PNG_HD bool png_tree_lengths(PngDeflateShared& S, int sbase, int nbase, int nsym) {
    int m = 0;
    for (int s = 0; s < nsym; s++) m += S.wfreq[sbase + s] != 0u;
    // m >= 2: the literal / length tree holds the end-of-block code and a literal or a length, the distance tree its dummy codes
    int li = 0, ni = m, next = m;
    for (int k = 0; k < m - 1; k++) {
        int pick[2];
        unsigned f = 0;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const bool leaf = li < m && (ni >= next || S.nfreq[nbase + li] <= S.nfreq[nbase + ni]);
            const int node = leaf ? li : ni;
            if (leaf) li++; else ni++;
            f += S.nfreq[nbase + node];
            if (j == 0) pick[0] = node; else pick[1] = node;
        }
        S.nfreq[nbase + next] = f;
        S.parent[nbase + pick[0]] = (unsigned short)next;
        S.parent[nbase + pick[1]] = (unsigned short)next;
        next++;
    }
    S.depth[nbase + 2 * m - 2] = 0;
    int maxd = 0;
    for (int k = 2 * m - 3; k >= 0; k--) {
        const int d = S.depth[nbase + S.parent[nbase + k]] + 1;
        S.depth[nbase + k] = (uint8_t)(d > 255 ? 255 : d);
        if (k < m && d > maxd) maxd = d;
    }
    if (maxd > 15) return false;
    for (int k = 0; k < m; k++) S.clen[sbase + S.sorted[sbase + k]] = S.depth[nbase + k];
    return true;
}

// one lane: canonical codes of one tree from its lengths, stored bit-reversed
PNG_HD void png_canonical(PngDeflateShared& S, int sbase, int nsym) {
    for (int b = 0; b < 16; b++) S.blc[b] = 0u;
    for (int s = 0; s < nsym; s++) S.blc[S.clen[sbase + s]]++;
    S.blc[0] = 0u;
    unsigned c = 0;
    for (int b = 1; b < 16; b++) { c = (c + S.blc[b - 1]) << 1; S.nextc[b] = c; }
    for (int s = 0; s < nsym; s++) {
        const int l = S.clen[sbase + s];
        S.code[sbase + s] = l ? (unsigned short)png_rev(S.nextc[l]++, l) : (unsigned short)0;
    }
}

__host__ __device__ inline void png_deflate_segment(PngDeflateShared& S, const PngEncParams& p, long s) {
    const long first = s * PE_SEG;
    const int n = (int)(p.total - first < PE_SEG ? p.total - first : PE_SEG);
    const bool last_seg = s == p.nseg - 1;
    const int nsub = (n + PE_SUB - 1) / PE_SUB;
    const int zoff = s == 0 ? 2 : 0;
    uint8_t* slot = p.slots + s * PE_SLOT;
    // load (the stream buffer is padded to whole 16-byte vectors)
    PNG_EACH_THREAD(tid, PE_THREADS) {
        const uint4* g = reinterpret_cast<const uint4*>(p.stream + first);
        uint4* d = reinterpret_cast<uint4*>(S.data);
        for (int i = tid; i < (n + 15) / 16; i += PE_THREADS) d[i] = g[i];
        for (int i = tid; i < PE_NSYM; i += PE_THREADS) { S.freq[i] = 0u; S.clen[i] = 0; S.code[i] = 0; }
        if (tid < PE_MAXC) S.cand[tid] = tid < p.ncand ? p.cand[tid] : 0x7fffffff;
        if (tid == 0) { S.adler_a = 0u; S.adler_b = 0ull; S.over = 0; }
    }
    // parse
    PNG_EACH_THREAD(tid, PE_THREADS) {
        for (int sb = tid; sb < nsub; sb += PE_THREADS) {
            int i = sb * PE_SUB;
            const int end = i + PE_SUB < n ? i + PE_SUB : n;
            unsigned a = 0;
            unsigned long long b = 0;
            for (int k = i; k < end; k++) { a += S.data[k]; b += a; }
            PNG_ATOMIC_ADD(&S.adler_a, a);
            PNG_ATOMIC_ADD(&S.adler_b, b + (unsigned long long)a * (unsigned)(n - end));
            while (i < end) {
                const int maxlen = end - i < 258 ? end - i : 258;
                int best = 0, bc = 0;
                if (maxlen >= 3 && p.mode != 1) {
                    const unsigned d0 = S.data[i], d1 = S.data[i + 1], d2 = S.data[i + 2];
                    for (int c = 0; c < PE_MAXC; c++) {
                        const int d = S.cand[c];
                        if (d > i) break;                                    // ascending: no later candidate fits either
                        const uint8_t* q = S.data + (i - d);
                        if (q[0] != d0 || q[1] != d1 || q[2] != d2) continue;
                        int l = 3;
                        while (l < maxlen && q[l] == S.data[i + l]) l++;
                        if (l > best && !(l == 3 && d > 4096)) {
                            best = l; bc = c;
                            if (l == maxlen) break;
                        }
                    }
                }
                if (best >= 3) {
                    S.tok[i] = (uint8_t)(bc + 1); S.tok[i + 1] = (uint8_t)(best - 3);
                    int sym, eb, ev;
                    png_len_code(best, sym, eb, ev);
                    PNG_ATOMIC_ADD(&S.freq[sym], 1u);
                    png_dist_code(S.cand[bc], sym, eb, ev);
                    PNG_ATOMIC_ADD(&S.freq[PE_DBASE + sym], 1u);
                    i += best;
                } else {
                    S.tok[i] = 0;
                    PNG_ATOMIC_ADD(&S.freq[S.data[i]], 1u);
                    i++;
                }
            }
        }
    }
    // the working frequencies: + end of block, + dummy distance codes so that two are in use
    PNG_EACH_THREAD(tid, PE_THREADS) {
        if (tid == 0) {
            S.freq[256] = 1u;
            int used = 0;
            for (int d = 0; d < 30; d++) used += S.freq[PE_DBASE + d] != 0u;
            for (int i = 0; i < PE_NSYM; i++) S.wfreq[i] = S.freq[i];
            for (int d = 0; d < 30 && used < 2; d++)
                if (S.wfreq[PE_DBASE + d] == 0u) { S.wfreq[PE_DBASE + d] = 1u; used++; }
        }
    }
    for (int round = 0; round < 32; round++) {
        // rank the used symbols of both trees by (frequency, index)
        PNG_EACH_THREAD(tid, PE_THREADS) {
            for (int x = tid; x < PE_NSYM; x += PE_THREADS) {
                S.clen[x] = 0;
                const unsigned f = S.wfreq[x];
                if (f == 0u) continue;
                const int lo = x < PE_DBASE ? 0 : PE_DBASE, hi = x < PE_DBASE ? PE_DBASE : PE_NSYM;
                int rank = 0;
                for (int y = lo; y < hi; y++) {
                    const unsigned g = S.wfreq[y];
                    rank += (g != 0u && (g < f || (g == f && y < x))) ? 1 : 0;
                }
                S.sorted[lo + rank] = (unsigned short)(x - lo);
                S.nfreq[2 * lo + rank] = f;
            }
        }
        PNG_EACH_THREAD(tid, PE_THREADS) {
            if (tid == 0) {
                const bool ok0 = png_tree_lengths(S, 0, 0, PE_DBASE);
                const bool ok1 = png_tree_lengths(S, PE_DBASE, 2 * PE_DBASE, 32);
                S.over = (ok0 && ok1) ? 0 : 1;
                if (S.over)
                    for (int i = 0; i < PE_NSYM; i++) S.wfreq[i] = (S.wfreq[i] + 1u) >> 1;
            }
        }
        PNG_SYNC();
        const int over = S.over;
        PNG_SYNC();
        if (!over) break;
    }
    // sizes and the choice
    PNG_EACH_THREAD(tid, PE_THREADS) {
        if (tid == 0) {
            unsigned long long dyn = 0, fix = 0;
            int hlit = 257, hdist = 1;
            for (int x = 0; x < PE_NSYM; x++) {
                const unsigned f = S.freq[x];
                const int e = png_sym_extra(x);
                dyn += (unsigned long long)f * (unsigned)(S.clen[x] + e);
                fix += (unsigned long long)f * (unsigned)(png_fixed_len(x) + e);
                if (S.clen[x]) { if (x < PE_DBASE) { if (x + 1 > hlit) hlit = x + 1; } else if (x - PE_DBASE + 1 > hdist) hdist = x - PE_DBASE + 1; }
            }
            const unsigned hdr_dyn = 3u + 14u + 57u + 4u * (unsigned)(hlit + hdist);
            const unsigned long long t_dyn = hdr_dyn + dyn + 3u, t_fix = 3u + fix + 3u;
            const unsigned long long b_dyn = (t_dyn + 7) / 8 + 4, b_fix = (t_fix + 7) / 8 + 4, b_sto = (unsigned long long)png_stored_bytes(n);
            int type = p.mode - 1;
            if (p.mode == 0) {
                type = 0;
                unsigned long long best = b_sto;
                if (b_fix < best) { best = b_fix; type = 1; }
                if (b_dyn < best) { best = b_dyn; type = 2; }
            }
            S.type = type; S.hlit = hlit; S.hdist = hdist;
            S.hdr_bits = type == 2 ? hdr_dyn : 3u;
            S.total_bits = (unsigned)(type == 2 ? t_dyn : t_fix);
            if (type == 1)
                for (int x = 0; x < PE_NSYM; x++) S.clen[x] = (uint8_t)png_fixed_len(x);
            if (type != 0) { png_canonical(S, 0, PE_DBASE); png_canonical(S, PE_DBASE, 32); }
            const long deflate_bytes = type == 0 ? (long)b_sto : (long)((S.total_bits + 7u) / 8u + 4u);
            int64_t* m = p.meta + s * PE_META;
            m[0] = first; m[1] = first + n; m[2] = type; m[3] = 12 + zoff + deflate_bytes + (last_seg ? 4 : 0);
            m[4] = S.adler_a % PE_ADLER; m[5] = (int64_t)(S.adler_b % PE_ADLER); m[6] = 0; m[7] = 0;
            if (s == 0) { slot[0] = 0x78; slot[1] = 0x01; }
        }
    }
    PNG_SYNC();
    const int type = S.type;
    uint8_t* z = slot + zoff;
    const long zcap = PE_SLOT - zoff;
    if (type == 0) {
        PNG_EACH_THREAD(tid, PE_THREADS) {
            const int nb = (n + 65534) / 65535;
            if (tid < nb) {
                const int len = n - tid * 65535 < 65535 ? n - tid * 65535 : 65535;
                uint8_t* h = z + (long)tid * 65540;
                h[0] = (last_seg && tid == nb - 1) ? 1 : 0;
                h[1] = (uint8_t)(len & 255); h[2] = (uint8_t)(len >> 8); h[3] = (uint8_t)(~len & 255); h[4] = (uint8_t)((~len >> 8) & 255);
            }
            for (int j = tid; j < n; j += PE_THREADS) z[j + 5 * (j / 65535 + 1)] = S.data[j];
            if (p.index && tid < nsub) png_index_be32(p, 12 + p.H + 4 * (s * PE_NSUB + tid), 0u);
        }
        return;
    }
    // bits per sub-block
    PNG_EACH_THREAD(tid, PE_THREADS) {
        for (int sb = tid; sb < nsub; sb += PE_THREADS) {
            int i = sb * PE_SUB;
            const int end = i + PE_SUB < n ? i + PE_SUB : n;
            unsigned bits = 0;
            while (i < end) {
                const int t = S.tok[i];
                if (t == 0) { bits += S.clen[S.data[i]]; i++; continue; }
                const int len = (int)S.tok[i + 1] + 3;
                int sym, eb, ev;
                png_len_code(len, sym, eb, ev);
                bits += S.clen[sym] + eb;
                png_dist_code(S.cand[(t - 1) % PE_MAXC], sym, eb, ev);
                bits += S.clen[PE_DBASE + sym] + eb;
                i += len;
            }
            S.bits[sb] = bits;
        }
    }
    PNG_EACH_THREAD(tid, PE_THREADS) {
        if (tid == 0) {
            unsigned o = S.hdr_bits;
            for (int sb = 0; sb < nsub; sb++) { S.off[sb] = o; o += S.bits[sb]; }
            S.off[nsub] = o;
        }
    }
    // emit
    PNG_EACH_THREAD(tid, PE_THREADS) {
        for (int sb = tid; sb < nsub; sb += PE_THREADS) {
            PngBitWriter w;
            w.base = z; w.cap = zcap; w.acc = 0ull; w.lim = 0x7fffffffffffffffL;
            if (p.index) png_index_be32(p, 12 + p.H + 4 * (s * PE_NSUB + sb), S.off[sb] + 8u * (unsigned)zoff);
            int i = sb * PE_SUB;
            const int end = i + PE_SUB < n ? i + PE_SUB : n;
            if (sb == 0) {
                w.pos = 0; w.n = 0; w.skip = -1;
                w.put(0u, 1);
                if (type == 1) {
                    w.put(1u, 2);
                } else {
                    w.put(2u, 2);
                    w.put((unsigned)(S.hlit - 257), 5); w.put((unsigned)(S.hdist - 1), 5); w.put(15u, 4);
                    for (int k = 0; k < 19; k++) w.put(k < 3 ? 0u : 4u, 3);      // order 16 17 18 0 8 7 ...: the first three are unused, every other one 4 bits
                    for (int k = 0; k < S.hlit; k++) w.put(png_rev(S.clen[k], 4), 4);
                    for (int k = 0; k < S.hdist; k++) w.put(png_rev(S.clen[PE_DBASE + k], 4), 4);
                }
            } else {
                const unsigned o = S.off[sb];
                w.pos = o >> 3; w.n = (int)(o & 7u); w.skip = w.n ? w.pos : -1;
            }
            while (i < end) i = png_put_token(S, w, i, n, last_seg);
            if (end == n) i = png_put_token(S, w, n, n, last_seg);
            if (w.n != 0 && w.pos != w.skip) {
                // the last byte is this lane's: fill it from the tokens that follow
                const long mine = w.pos;
                w.lim = mine + 1;
                while (w.pos <= mine && i <= n) i = png_put_token(S, w, i, n, last_seg);
            }
        }
        if (tid == 0) {
            const long e = (S.total_bits + 7u) / 8u;
            if (e + 4 <= zcap) { z[e] = 0; z[e + 1] = 0; z[e + 2] = 0xff; z[e + 3] = 0xff; }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// (c) chunks and checksums

constexpr unsigned PE_POLY = 0xedb88320u;
// a(x) b(x) modulo the CRC-32 polynomial, reflected: bit 31 is x^0 (the arithmetic of zlib's crc32_combine)
PNG_HD unsigned png_multmodp(unsigned a, unsigned b) {
    unsigned m = 1u << 31, r = 0;
    for (int i = 0; i < 32; i++) {
        if (a & m) r ^= b;
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ PE_POLY : b >> 1;
    }
    return r;
}

struct PngAsmShared {
    uint8_t stage[PE_PIECE];
    unsigned tab[256];
    unsigned x2n[32];                         // x^(2^k) modulo the polynomial
    unsigned crc[PE_ASM_THREADS];
    unsigned len[PE_ASM_THREADS];
    unsigned long long sum_off, ad_a, ad_b;
    unsigned crc_total, adler;
    long off, plen;
};

PNG_HD unsigned png_x8n(const PngAsmShared& S, unsigned long long nbytes) {      // x^(8 n)
    unsigned r = 1u << 31;
    unsigned k = 3;
    while (nbytes) {
        if (nbytes & 1ull) r = png_multmodp(S.x2n[k & 31u], r);
        nbytes >>= 1; k++;
    }
    return r;
}
PNG_HD unsigned png_crc_join(const PngAsmShared& S, unsigned crc1, unsigned crc2, unsigned long long len2) { return png_multmodp(png_x8n(S, len2), crc1) ^ crc2; }
PNG_HD unsigned png_crc_bytes(const PngAsmShared& S, const uint8_t* b, int n) {
    unsigned c = 0xffffffffu;
    for (int i = 0; i < n; i++) c = S.tab[(c ^ b[i]) & 255u] ^ (c >> 8);
    return c ^ 0xffffffffu;
}
PNG_HD void png_out(const PngEncParams& p, long at, unsigned v) { if (at >= 0 && at < p.out_cap) p.out[at] = (uint8_t)v; }
PNG_HD void png_out_be32(const PngEncParams& p, long at, unsigned v) { png_out(p, at, v >> 24); png_out(p, at + 1, (v >> 16) & 255u); png_out(p, at + 2, (v >> 8) & 255u); png_out(p, at + 3, v & 255u); }

// s == p.nseg (launched only with an index): the ldIX chunk, framed like a segment's IDAT
__host__ __device__ inline void png_assemble_segment(PngAsmShared& S, const PngEncParams& p, long s) {
    const bool last_seg = s == p.nseg - 1, is_index = s == p.nseg;
    const uint8_t* slot = is_index ? p.index : p.slots + s * PE_SLOT;
    const long index_chunk = p.index ? 12 + p.index_bytes : 0;
    PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
        unsigned c = (unsigned)tid;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PE_POLY : c >> 1;
        S.tab[tid] = c;
        if (tid == 0) {
            unsigned v = 1u << 30;
            S.x2n[0] = v;
            for (int k = 1; k < 32; k++) { v = png_multmodp(v, v); S.x2n[k] = v; }
            S.sum_off = 0ull; S.ad_a = 0ull; S.ad_b = 0ull; S.crc_total = 0u;
        }
    }
    PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
        unsigned long long so = 0, a = 0, b = 0;
        for (long j = tid; j < p.nseg; j += PE_ASM_THREADS) {
            const int64_t* m = p.meta + j * PE_META;
            if (j < s) so += (unsigned long long)png_clampl(m[3], 12, 12 + PE_SLOT + 4);
            if (last_seg) {
                const unsigned long long aj = (unsigned long long)png_clampl(m[4], 0, PE_ADLER - 1), bj = (unsigned long long)png_clampl(m[5], 0, PE_ADLER - 1);
                const long end = j * PE_SEG + PE_SEG < p.total ? j * PE_SEG + PE_SEG : p.total;
                a += aj; b += bj + aj * (unsigned long long)(p.total - end);
            }
        }
        PNG_ATOMIC_ADD(&S.sum_off, so);
        if (last_seg) { PNG_ATOMIC_ADD(&S.ad_a, a); PNG_ATOMIC_ADD(&S.ad_b, b); }
    }
    PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
        if (tid == 0) {
            S.off = is_index ? PE_FILE_HEAD : PE_FILE_HEAD + index_chunk + (long)S.sum_off;
            if (is_index) {
                S.plen = p.index_bytes;
            } else {
                S.plen = png_clampl(p.meta[s * PE_META + 3], 12, 12 + PE_SLOT + 4) - 12 - (last_seg ? 4 : 0);     // payload bytes that sit in the slot
                S.plen = png_clampl(S.plen, 0, PE_SLOT);
            }
            const unsigned A = (unsigned)((1ull + S.ad_a) % PE_ADLER), B = (unsigned)(((unsigned long long)p.total + S.ad_b) % PE_ADLER);
            S.adler = (B << 16) | A;
        }
    }
    PNG_SYNC();
    const long off = S.off, plen = S.plen;
    const long body = 4 + plen + (last_seg ? 4 : 0);                                                            // type + payload: what the CRC covers
    const unsigned adler = S.adler;
    for (long p0 = 0; p0 < body; p0 += PE_PIECE) {
        const int len = (int)(body - p0 < PE_PIECE ? body - p0 : PE_PIECE);
        PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
            for (int k = tid; k < len; k += PE_ASM_THREADS) {
                const long q = p0 + k;
                unsigned v;
                if (q < 4) v = is_index ? (q == 0 ? 'l' : (q == 1 ? 'd' : (q == 2 ? 'I' : 'X'))) : (q == 0 ? 'I' : (q == 1 ? 'D' : (q == 2 ? 'A' : 'T')));
                else if (q < 4 + plen) v = slot[q - 4];
                else v = (adler >> (8 * (3 - (q - 4 - plen)))) & 255u;
                S.stage[k] = (uint8_t)v;
                png_out(p, off + 4 + q, v);
            }
        }
        PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
            const int b0 = tid * PE_SLICE;
            const int m = len - b0 < 0 ? 0 : (len - b0 < PE_SLICE ? len - b0 : PE_SLICE);
            S.crc[tid] = m ? png_crc_bytes(S, S.stage + b0, m) : 0u;
            S.len[tid] = (unsigned)m;
        }
        for (int stride = 1; stride < PE_ASM_THREADS; stride *= 2) {
            PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
                if (tid % (2 * stride) == 0) {
                    S.crc[tid] = png_crc_join(S, S.crc[tid], S.crc[tid + stride], S.len[tid + stride]);
                    S.len[tid] += S.len[tid + stride];
                }
            }
        }
        PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
            if (tid == 0) S.crc_total = png_crc_join(S, S.crc_total, S.crc[0], (unsigned long long)len);
        }
    }
    PNG_EACH_THREAD(tid, PE_ASM_THREADS) {
        if (tid == 0) {
            png_out_be32(p, off, (unsigned)(body - 4));
            png_out_be32(p, off + 4 + body, S.crc_total);
            if (p.user_table && !is_index) {
                const int64_t* m = p.meta + s * PE_META;
                int64_t* u = p.user_table + 4 * s;
                u[0] = m[0]; u[1] = m[1]; u[2] = m[2]; u[3] = 12 + body - 4;
            }
            if (s == 0) {
                const unsigned long long sig = 0x0a1a0a0d474e5089ull;                                           // 89 'P' 'N' 'G' 0d 0a 1a 0a
                for (int k = 0; k < 8; k++) png_out(p, k, (unsigned)(sig >> (8 * k)) & 255u);
                // IHDR: 8-bit RGB, no interlace
                uint8_t* h = S.stage;                                                                           // (every piece has been consumed)
                h[0] = 'I'; h[1] = 'H'; h[2] = 'D'; h[3] = 'R';
                for (int k = 0; k < 4; k++) { h[4 + k] = (uint8_t)((unsigned)p.W >> (8 * (3 - k))); h[8 + k] = (uint8_t)((unsigned)p.H >> (8 * (3 - k))); }
                h[12] = 8; h[13] = 2; h[14] = 0; h[15] = 0; h[16] = 0;
                png_out_be32(p, 8, 13u);
                for (int k = 0; k < 17; k++) png_out(p, 12 + k, h[k]);
                png_out_be32(p, 29, png_crc_bytes(S, h, 17));
            }
            if (last_seg) {
                const long e = off + 8 + body;
                uint8_t* h = S.stage + 32;
                h[0] = 'I'; h[1] = 'E'; h[2] = 'N'; h[3] = 'D';
                png_out_be32(p, e, 0u);
                for (int k = 0; k < 4; k++) png_out(p, e + 4 + k, h[k]);
                png_out_be32(p, e + 8, png_crc_bytes(S, h, 4));
                const long total = e + 12;
                *p.out_total = total <= p.out_cap ? total : -total;                                             // negative: the file did not fit (a forced block mode)
            }
        }
    }
}

__global__ void __launch_bounds__(PE_FILTER_THREADS) png_enc_filter_kernel(PngEncParams p) {
    __shared__ PngFilterShared S;
    png_filter_row(S, p, (long)blockIdx.x);
}
__global__ void __launch_bounds__(PE_THREADS) png_enc_deflate_kernel(PngEncParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char png_enc_lds[];
    png_deflate_segment(*reinterpret_cast<PngDeflateShared*>(png_enc_lds), p, (long)blockIdx.x);
}
__global__ void __launch_bounds__(PE_ASM_THREADS) png_enc_assemble_kernel(PngEncParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char png_asm_lds[];
    png_assemble_segment(*reinterpret_cast<PngAsmShared*>(png_asm_lds), p, (long)blockIdx.x);
}

static inline int64_t pe_round16(int64_t v) { return (v + 15) / 16 * 16; }

// workspace layout: stream | segment table | slots, each 16-byte aligned
struct PngEncLayout { int64_t total, nseg, stream_bytes, meta_off, slots_off, workspace, bound, index_bytes; };

static inline PngEncLayout png_enc_layout(int H, int W) {
    PngEncLayout l;
    l.total = (int64_t)H * (1 + 3 * (int64_t)W);
    l.nseg = (l.total + PE_SEG - 1) / PE_SEG;
    l.stream_bytes = pe_round16(l.total) + 16;
    l.meta_off = l.stream_bytes;
    l.slots_off = l.meta_off + pe_round16(l.nseg * PE_META * 8);
    l.workspace = l.slots_off + l.nseg * PE_SLOT;
    const int64_t tail = l.total - (l.nseg - 1) * PE_SEG;
    l.bound = PE_FILE_HEAD + 2 + (l.nseg - 1) * (12 + png_stored_bytes(PE_SEG)) + 12 + png_stored_bytes(tail) + 4 + 12;
    l.index_bytes = 12 + H + 4 * ((l.nseg - 1) * PE_NSUB + (tail + PE_SUB - 1) / PE_SUB);     // the ldIX payload, behind the slots in the workspace
    return l;
}

// the candidate distances of a row length, ascending and distinct
static inline int png_enc_candidates(int W, int* cand) {
    const long row = 1 + 3L * W;
    const long all[11] = {1, 2, 3, 4, 6, 9, 12, row - 3, row, row + 3, 2 * row};
    int n = 0;
    for (int i = 0; i < 11; i++) {
        const long d = all[i];
        if (d < 1 || d > 32768) continue;
        int at = 0;
        bool dup = false;
        for (int k = 0; k < n; k++) { if (cand[k] == d) dup = true; if (cand[k] < d) at = k + 1; }
        if (dup) continue;
        for (int k = n; k > at; k--) cand[k] = cand[k - 1];
        cand[at] = (int)d;
        n++;
    }
    return n;
}

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_png_encode_bound(int H, int W, int64_t* out_bytes, int64_t* workspace_bytes) {
    LDETR_CHECK(W >= 1 && W <= PE_MAX_DIM && H >= 1 && H <= PE_MAX_DIM, "png_encode: grid %d x %d outside [1, %d] x [1, %d]", W, H, PE_MAX_DIM, PE_MAX_DIM);
    const PngEncLayout l = png_enc_layout(H, W);
    if (out_bytes) *out_bytes = l.bound;
    if (workspace_bytes) *workspace_bytes = l.workspace;
    return LDETR_OK;
}

extern "C" int ldetr_png_index_bytes(int H, int W, int64_t* bytes) {
    LDETR_CHECK(W >= 1 && W <= PE_MAX_DIM && H >= 1 && H <= PE_MAX_DIM, "png_index_bytes: grid %d x %d outside [1, %d] x [1, %d]", W, H, PE_MAX_DIM, PE_MAX_DIM);
    LDETR_CHECK(bytes, "png_index_bytes: null pointer");
    *bytes = pe_round16(12 + png_enc_layout(H, W).index_bytes);
    return LDETR_OK;
}

extern "C" int ldetr_png_encode_u8(const ldetr_png_encode_args* a, void* stream) {
    LDETR_CHECK_BLOCK(a, ldetr_png_encode_args, "png_encode");
    const int H = a->H, W = a->W;
    LDETR_CHECK(W >= 1 && W <= PE_MAX_DIM && H >= 1 && H <= PE_MAX_DIM, "png_encode: grid %d x %d outside [1, %d] x [1, %d]", W, H, PE_MAX_DIM, PE_MAX_DIM);
    LDETR_CHECK(a->blocks >= 0 && a->blocks <= 3, "png_encode: blocks %d (0 auto, 1 stored, 2 fixed, 3 dynamic)", a->blocks);
    LDETR_CHECK(a->filter >= -1 && a->filter <= 4, "png_encode: filter %d (-1 auto, 0 .. 4)", a->filter);
    LDETR_CHECK(a->src && a->out && a->total_bytes && a->workspace, "png_encode: null pointer");
    LDETR_CHECK((a->reserved & ~1) == 0, "png_encode: reserved %d (bit 0: write the ldIX index chunk)", a->reserved);
    PngEncLayout l = png_enc_layout(H, W);
    const bool index = a->reserved & 1;
    if (index) {                                                                                                    // both buffers grow by ldetr_png_index_bytes
        const int64_t extra = pe_round16(12 + l.index_bytes);
        l.bound += extra; l.workspace += extra;
    }
    LDETR_CHECK(a->out_capacity >= l.bound, "png_encode: the output buffer holds %ld bytes, a %d x %d grid needs %ld (ldetr_png_encode_bound%s)", (long)a->out_capacity, W, H, (long)l.bound,
                index ? " + ldetr_png_index_bytes" : "");
    LDETR_CHECK(((uintptr_t)a->workspace & 15) == 0 && a->workspace_bytes >= l.workspace, "png_encode: the workspace must be 16-byte aligned and hold %ld bytes (got %ld)", (long)l.workspace,
                (long)a->workspace_bytes);
    LDETR_CHECK(!a->seg_table || a->seg_table_rows >= l.nseg, "png_encode: the segment table holds %ld rows, %ld needed", (long)a->seg_table_rows, (long)l.nseg);
    PngEncParams p;
    p.src = a->src; p.H = H; p.W = W; p.mode = a->blocks; p.filter = a->filter;
    p.stream = a->workspace; p.meta = reinterpret_cast<int64_t*>(a->workspace + l.meta_off); p.slots = a->workspace + l.slots_off;
    p.nseg = l.nseg; p.total = l.total; p.out = a->out; p.out_cap = a->out_capacity; p.out_total = a->total_bytes; p.user_table = a->seg_table;
    p.index = index ? a->workspace + l.slots_off + l.nseg * PE_SLOT : nullptr; p.index_bytes = index ? l.index_bytes : 0;
    p.ncand = png_enc_candidates(W, p.cand);
    for (int i = p.ncand; i < PE_MAXC; i++) p.cand[i] = 0x7fffffff;
    {
        LDETR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(png_enc_deflate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PngDeflateShared)) == hipSuccess &&
                        hipFuncSetAttribute(reinterpret_cast<const void*>(png_enc_assemble_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PngAsmShared)) == hipSuccess,
                    "png_encode: the device does not grant %d bytes of LDS per workgroup", (int)sizeof(PngDeflateShared));
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_enc_filter_kernel, dim3((unsigned)H), PE_FILTER_THREADS, 0, st, p);
    int rc = check_launch("png_encode (filter)");
    if (rc) return rc;
    hipLaunchKernelGGL(png_enc_deflate_kernel, dim3((unsigned)l.nseg), PE_THREADS, sizeof(PngDeflateShared), st, p);
    rc = check_launch("png_encode (deflate)");
    if (rc) return rc;
    hipLaunchKernelGGL(png_enc_assemble_kernel, dim3((unsigned)(l.nseg + (index ? 1 : 0))), PE_ASM_THREADS, sizeof(PngAsmShared), st, p);
    return check_launch("png_encode (assemble)");
}
