// The body of png_inflate_kernel (png_inflate.hip): one segment of an indexed page PNG inflated by one workgroup.
// Written, like png_encode.hip, as phases of "every thread does this" separated by workgroup barriers (PNG_EACH_THREAD): compiled for the host a phase
// is a loop over the thread index, which is how tools/png_inflate_hostcheck.cpp runs this very source under the sanitizers, corrupted files included.
// Nothing here needs the HIP headers.
//
// A segment is PI_SEG = 64 KiB of the filtered scanline stream, cut into sub-blocks of PI_SUB = 512 bytes; the file's ldIX chunk holds, per sub-block, the
// bit offset of its first token inside the segment's IDAT chunk, and no token crosses a sub-block.  Lane k decodes sub-block k:
//   header    lane 0 reads the block header; a dynamic block's code lengths (flat: 4 bits each) are read by all lanes, the canonical decode tables
//             (count per length + symbols in code order, 15 steps at most per symbol, no big lookup table) are built in LDS by lane 0.
//   pass 0    every lane decodes its tokens.  Literals go to LDS.  A match whose source bytes are all written copies at once (sources inside the lane's own
//             sub-block are); any other match is left PENDING: its (distance, length) is parked in the first three of the bytes it will produce -- they
//             are unwritten, and a match is at least three bytes long -- so pending matches need no storage of their own.
//   rounds    every lane walks the unwritten bytes of its sub-block (a bitmap, 16 words per lane, owned by that lane: no atomics) and retries the matches
//             parked there.  Sources in other sub-blocks are tested against the bitmap AS IT WAS WHEN THE ROUND BEGAN (`written`), sources in the lane's own
//             sub-block against the live one (`fresh`); `fresh` is copied to `written` between rounds.  So what a round does depends on no timing, and host
//             and device agree.  Sub-block k is complete after round k at the latest (its sources lie in sub-blocks <= k), hence at most nsub rounds; a round
//             that resolves nothing while something is pending ends the loop with PI_ERR_STUCK.  Nothing spins.
//   output    the segment goes to the dense stream with aligned dword stores (bytes at the two ends); the filter bytes inside it are compared to the index.
// Every bit position is clamped to the file's dwords, every table index, distance and output index is range-checked before use: a corrupt file or a stale
// table gives an error bit and wrong bytes, never an access outside the file buffer, the stream buffer or LDS.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNGI_HD __host__ __device__ __forceinline__
#else
#define PNGI_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGI_EACH_THREAD(tid, nt) __syncthreads(); for (int tid = threadIdx.x, once_ = 1; once_; once_ = 0)
#define PNGI_SYNC() __syncthreads()
#define PNGI_OR(ptr, v) atomicOr((ptr), (v))
#else
#define PNGI_EACH_THREAD(tid, nt) for (int tid = 0; tid < (nt); tid++)
#define PNGI_SYNC() do {} while (0)
#define PNGI_OR(ptr, v) (*(ptr) |= (v))
#endif

namespace ldetr {

constexpr int PI_SEG = 65536;                  // = PE_SEG of png_encode.hip
constexpr int PI_SUB = 512;                    // = PE_SUB
constexpr int PI_NSUB = PI_SEG / PI_SUB;
constexpr int PI_THREADS = 128;                // one lane per sub-block
constexpr int PI_WORDS = PI_SUB / 32;          // bitmap words per sub-block

// the status word of a page (include/ldetr_hip.h LDETR_PNG_INFLATE_*)
constexpr int PI_ERR_CODE = 1;                 // an invalid Huffman code, code-length set or block header
constexpr int PI_ERR_COUNT = 2;                // a sub-block that did not yield its byte count exactly, or did not end at the next index entry
constexpr int PI_ERR_HEADER = 4;               // the block header did not end at index entry 0
constexpr int PI_ERR_DISTANCE = 8;             // a distance that reaches before the segment start
constexpr int PI_ERR_TRAILER = 16;             // no end-of-block code, or no empty stored block up to the end of the chunk
constexpr int PI_ERR_FILTER = 32;              // a filter byte of the stream differs from the index
constexpr int PI_ERR_STUCK = 64;               // matches left unresolved
constexpr int PI_ERR_TABLE = 128;              // a segment table entry that leaves its file

struct PngInflateParams {
    const uint8_t* files; long files_bytes;        // the files, each 16-byte aligned; files_bytes a multiple of 16
    const int64_t* file_off;                       // [n + 1]
    const int64_t* seg;                            // [n][nseg][4] = (offset of the IDAT chunk's data in its file, bytes, kind 0 stored / 1 fixed / 2 dynamic, first index entry)
    const int64_t* index_off;                      // [n]: offset of the ldIX chunk's data in its file
    uint8_t* stream; long stream_bytes;            // [n][H (1 + 3 W)]
    int32_t* status;                               // [n], zero before the launch; a workgroup that found an error stores its bits
    int n, H, W;
    long nseg, total;                              // per page: ceil(total / PI_SEG), H (1 + 3 W)
};

struct PngInflateShared {
    uint8_t out[PI_SEG];
    uint32_t written[PI_SEG / 32];                 // one bit per output byte, as of the start of the round
    uint32_t fresh[PI_SEG / 32];                   // the live one; a lane touches its own PI_WORDS words only
    uint16_t lsym[288], dsym[32];                  // symbols in canonical code order
    uint16_t lcount[16], dcount[16];               // codes per length
    uint16_t offs[16];                             // lane 0's cursor per length while it builds a table
    uint8_t len[320];                              // code lengths: literal / length at 0, distance at 288
    int status, pending, progress, bad;
    int hlit, hdist;
    long hdr_end;                                  // absolute bit position behind the block header
};

PNGI_HD long pngi_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// LSB-first bit reader over the aligned dwords of one file; every dword index is clamped to the file
struct PngBitReader {
    const uint32_t* words;
    long w_lo, w_hi;
    unsigned long long acc;
    int cnt;
    long next;
    PNGI_HD uint32_t load(long i) const { return words[pngi_clampl(i, w_lo, w_hi)]; }
    PNGI_HD void seek(long bit) {
        next = bit >> 5;
        acc = (unsigned long long)load(next) >> (bit & 31);
        cnt = 32 - (int)(bit & 31);
        next++;
    }
    PNGI_HD void need() {                          // afterwards at least 33 bits are there
        if (cnt <= 32) { acc |= (unsigned long long)load(next) << cnt; cnt += 32; next++; }
    }
    PNGI_HD unsigned peek(int n) const { return (unsigned)(acc & ((1ull << n) - 1ull)); }       // n <= 32
    PNGI_HD void skip(int n) { acc >>= n; cnt -= n; }
    PNGI_HD unsigned get(int n) { const unsigned v = peek(n); skip(n); return v; }
    PNGI_HD long pos() const { return next * 32 - cnt; }
};

// one canonical Huffman symbol (at least 15 bits are in the reader); -1: no code matches.  The index into sym stays below the sum of the counts.
PNGI_HD int pngi_symbol(PngBitReader& br, const uint16_t* count, const uint16_t* sym, int nsym) {
    const unsigned v = br.peek(15);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; l++) {
        code |= (int)((v >> (l - 1)) & 1u);
        const int c = count[l];
        if (code - first < c) {
            br.skip(l);
            const int at = index + (code - first);
            return (at >= 0 && at < nsym) ? sym[at] : -1;                        // (an over-subscribed set can put code below first)
        }
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    return -1;
}

// lane 0: decode tables of one code from its lengths; false for an over-subscribed set
PNGI_HD bool pngi_build(const uint8_t* len, int n, uint16_t* count, uint16_t* sym, uint16_t* offs) {
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[len[s] & 15]++;
    count[0] = 0;
    int left = 1;
    bool ok = true;
    for (int l = 1; l < 16; l++) { left = 2 * left - count[l]; if (left < 0) { ok = false; left = 0; } }
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = offs[l] + count[l];
    for (int s = 0; s < n; s++) {
        const int l = len[s] & 15;
        if (l) sym[offs[l]++] = (uint16_t)s;
    }
    return ok;
}

PNGI_HD bool pngi_all_set(const uint32_t* bm, int a, int b) {                   // bits [a, b), 0 <= a < b <= PI_SEG
    for (int w = a >> 5; w <= (b - 1) >> 5; w++) {
        uint32_t m = 0xffffffffu;
        if (w == a >> 5) m &= 0xffffffffu << (a & 31);
        if (w == (b - 1) >> 5) m &= 0xffffffffu >> (31 - ((b - 1) & 31));
        if ((bm[w] & m) != m) return false;
    }
    return true;
}
PNGI_HD void pngi_set(uint32_t* bm, int a, int b) {                             // the caller's own words
    for (int w = a >> 5; w <= (b - 1) >> 5; w++) {
        uint32_t m = 0xffffffffu;
        if (w == a >> 5) m &= 0xffffffffu << (a & 31);
        if (w == (b - 1) >> 5) m &= 0xffffffffu >> (31 - ((b - 1) & 31));
        bm[w] |= m;
    }
}

// the len bytes of a match at dst, as byte-by-byte copying from dst - dist gives them (dist < len repeats).  One lane copies alone and a byte at a time each
// read waits for LDS before the next write can follow: a run (dist 1) is one read, and a group of up to 8 bytes no write of the group reaches (dist >= the
// group) is read before it is written, so the reads are in flight together
PNGI_HD void pngi_copy(uint8_t* out, int dst, int len, int dist) {
    const int src = dst - dist;
    int j = 0;
    if (dist == 1) {
        const uint8_t v = out[src];
        for (; j < len; j++) out[dst + j] = v;
        return;
    }
    if (dist >= 8) {
        for (; j + 8 <= len; j += 8) {
            const uint8_t b0 = out[src + j], b1 = out[src + j + 1], b2 = out[src + j + 2], b3 = out[src + j + 3], b4 = out[src + j + 4], b5 = out[src + j + 5], b6 = out[src + j + 6],
                          b7 = out[src + j + 7];
            out[dst + j] = b0; out[dst + j + 1] = b1; out[dst + j + 2] = b2; out[dst + j + 3] = b3; out[dst + j + 4] = b4; out[dst + j + 5] = b5; out[dst + j + 6] = b6; out[dst + j + 7] = b7;
        }
    }
    for (; j < len; j++) out[dst + j] = out[src + j];
}

// a match of len bytes at i from distance dist (1 <= dist <= i, i + len inside the lane's sub-block that starts at `start`): copy it if every source
// byte it does not produce itself is written
PNGI_HD bool pngi_try_copy(PngInflateShared& S, int start, int i, int len, int dist) {
    const int src = i - dist, src_end = src + len < i ? src + len : i;
    if (src < start) {
        if (!pngi_all_set(S.written, src, src_end < start ? src_end : start)) return false;
        if (src_end > start && !pngi_all_set(S.fresh, start, src_end)) return false;
    } else if (!pngi_all_set(S.fresh, src, src_end)) {
        return false;
    }
    pngi_copy(S.out, i, len, dist);
    pngi_set(S.fresh, i, i + len);
    return true;
}

PNGI_HD void pngi_zero(PngInflateShared& S, int a, int b) {
    if (a >= b) return;
    for (int j = a; j < b; j++) S.out[j] = 0;
    pngi_set(S.fresh, a, b);
}

PNGI_HD unsigned pngi_file_be32(const PngInflateParams& p, long f0, long f1, long at) {      // four bytes of the file [f0, f1), clamped
    unsigned v = 0;
    for (int k = 0; k < 4; k++) v = (v << 8) | p.files[pngi_clampl(f0 + at + k, f0, f1 - 1)];
    return v;
}

#if defined(__HIPCC__)
__host__ __device__
#endif
inline void png_inflate_segment(PngInflateShared& S, const PngInflateParams& p, long page, long s) {
    const long first = s * PI_SEG;
    const int n = (int)(p.total - first < PI_SEG ? p.total - first : PI_SEG);
    const int nsub = (n + PI_SUB - 1) / PI_SUB;
    const bool last_seg = s == p.nseg - 1;
    const long f0 = pngi_clampl(p.file_off[page], 0, p.files_bytes - 1), f1 = pngi_clampl(p.file_off[page + 1], f0 + 1, p.files_bytes);
    const int64_t* q = p.seg + 4 * (page * p.nseg + s);
    const long flen = f1 - f0;
    const long c_off = pngi_clampl(q[0], 0, flen - 1), c_len = pngi_clampl(q[1], 1, flen - c_off);
    const int kind = (int)pngi_clampl(q[2], 0, 2);
    const long entry0 = pngi_clampl(q[3], 0, 0x7fffffff);
    const long ix = pngi_clampl(p.index_off[page], 0, flen - 1);
    const long zoff = s == 0 ? 2 : 0;
    const long base_bit = 8 * (f0 + c_off);                                     // of the chunk's first data byte, in the file buffer
    const long chunk_bits = 8 * c_len;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(p.files);
    const long w_lo = f0 >> 2, w_hi = (f1 - 1) >> 2;

    PNGI_EACH_THREAD(tid, PI_THREADS) {
        for (int w = tid; w < PI_SEG / 32; w += PI_THREADS) { S.written[w] = 0u; S.fresh[w] = 0u; }
        for (int k = tid; k < 320; k += PI_THREADS) S.len[k] = 0;
        if (tid == 0) {
            S.status = (q[0] != c_off || q[1] != c_len || q[2] != kind || q[3] != entry0 || p.index_off[page] != ix) ? PI_ERR_TABLE : 0;
            S.pending = 0; S.progress = 0; S.bad = 0; S.hlit = 0; S.hdist = 0; S.hdr_end = 0;
        }
    }
    // bytes behind the segment's end count as written: a complete sub-block is PI_WORDS full words
    PNGI_EACH_THREAD(tid, PI_THREADS) {
        if (tid == 0 && n < PI_SEG) pngi_set(S.fresh, n, PI_SEG);
    }
    if (kind == 0) {
        // the stored form: blocks of at most 65535 bytes behind 5-byte headers (the host scan checked them)
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            for (int j = tid; j < n; j += PI_THREADS) S.out[j] = p.files[pngi_clampl(f0 + c_off + zoff + j + 5 * (j / 65535 + 1), f0, f1 - 1)];
        }
    } else {
        // block header
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            if (tid == 0) {
                PngBitReader br;
                br.words = words; br.w_lo = w_lo; br.w_hi = w_hi;
                br.seek(base_bit + 8 * zoff);
                br.need();
                const unsigned h = br.get(3);
                int err = 0;
                if ((h & 1u) != 0u || (int)(h >> 1) != kind) err |= PI_ERR_CODE;
                if (kind == 2) {
                    const int hlit = 257 + (int)br.get(5), hdist = 1 + (int)br.get(5), hclen = (int)br.get(4);
                    if (hlit > 286 || hdist > 30 || hclen != 15) err |= PI_ERR_CODE;
                    for (int k = 0; k < 19; k++) {                              // the flat code-length code: 16, 17, 18 unused, 4 bits for 0 .. 15
                        br.need();
                        if (br.get(3) != (k < 3 ? 0u : 4u)) err |= PI_ERR_CODE;
                    }
                    S.hlit = hlit; S.hdist = hdist;
                    S.hdr_end = br.pos() + 4L * (hlit + hdist);
                } else {
                    S.hdr_end = br.pos();
                }
                if (err) { S.bad = 1; S.status |= err; }
            }
        }
        PNGI_SYNC();
        const int hlit = S.hlit, hdist = S.hdist;                               // <= 288, <= 32
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            if (kind == 2) {
                for (int k = tid; k < hlit + hdist; k += PI_THREADS) {
                    PngBitReader br;
                    br.words = words; br.w_lo = w_lo; br.w_hi = w_hi;
                    br.seek(S.hdr_end - 4L * (hlit + hdist - k));
                    br.need();
                    const unsigned v = br.peek(4);                              // the 4-bit code of a length, first bit = its top bit
                    const unsigned l = ((v & 1u) << 3) | ((v & 2u) << 1) | ((v & 4u) >> 1) | ((v & 8u) >> 3);
                    S.len[k < hlit ? k : 288 + (k - hlit)] = (uint8_t)l;
                }
            } else {
                for (int k = tid; k < 320; k += PI_THREADS) S.len[k] = (uint8_t)(k >= 288 ? (k < 318 ? 5 : 0) : (k < 144 ? 8 : (k < 256 ? 9 : (k < 280 ? 7 : 8))));
            }
        }
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            if (tid == 0) {
                const bool ok0 = pngi_build(S.len, 288, S.lcount, S.lsym, S.offs), ok1 = pngi_build(S.len + 288, 32, S.dcount, S.dsym, S.offs);
                int err = (ok0 && ok1) ? 0 : PI_ERR_CODE;
                if (S.hdr_end - base_bit != (long)pngi_file_be32(p, f0, f1, ix + 12 + p.H + 4 * entry0)) err |= PI_ERR_HEADER;
                if (err) { S.bad = 1; S.status |= err; }
            }
        }
        PNGI_SYNC();
        const int bad = S.bad;
        // pass 0
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            if (tid < nsub) {
                const int start = tid * PI_SUB, end = start + PI_SUB < n ? start + PI_SUB : n;
                int i = start, err = 0, pend = 0;
                if (!bad) {
                    const long e_this = (long)pngi_file_be32(p, f0, f1, ix + 12 + p.H + 4 * (entry0 + tid));
                    PngBitReader br;
                    br.words = words; br.w_lo = w_lo; br.w_hi = w_hi;
                    br.seek(base_bit + pngi_clampl(e_this, 0, chunk_bits));
                    while (i < end) {
                        br.need();
                        int sym = pngi_symbol(br, S.lcount, S.lsym, 288);
                        if (sym < 0 || sym > 285) { err |= PI_ERR_CODE; break; }
                        if (sym < 256) {
                            S.out[i] = (uint8_t)sym;
                            S.fresh[i >> 5] |= 1u << (i & 31);
                            i++;
                            continue;
                        }
                        if (sym == 256) { err |= PI_ERR_COUNT; break; }
                        sym -= 257;
                        int len;
                        if (sym < 8) len = 3 + sym;
                        else if (sym == 28) len = 258;
                        else { const int e = (sym - 4) >> 2; len = 3 + ((4 + (sym & 3)) << e) + (int)br.get(e); }
                        br.need();
                        const int d = pngi_symbol(br, S.dcount, S.dsym, 32);
                        if (d < 0 || d > 29) { err |= PI_ERR_CODE; break; }
                        int dist;
                        if (d < 4) dist = 1 + d;
                        else { const int e = (d >> 1) - 1; dist = 1 + ((2 + (d & 1)) << e) + (int)br.get(e); }
                        if (i + len > end) { err |= PI_ERR_COUNT; break; }
                        if (dist > i) { err |= PI_ERR_DISTANCE; break; }
                        if (!pngi_try_copy(S, start, i, len, dist)) {
                            const unsigned rec = (unsigned)(dist - 1) | ((unsigned)(len - 3) << 15);
                            S.out[i] = (uint8_t)rec; S.out[i + 1] = (uint8_t)(rec >> 8); S.out[i + 2] = (uint8_t)(rec >> 16);
                            pend = 1;
                        }
                        i += len;
                    }
                    if (!err) {
                        if (tid + 1 < nsub) {
                            if (br.pos() - base_bit != (long)pngi_file_be32(p, f0, f1, ix + 12 + p.H + 4 * (entry0 + tid + 1))) err |= PI_ERR_COUNT;
                        } else {
                            // end of block, the empty stored block, the end of the chunk (the Adler-32 behind the last one)
                            br.need();
                            bool ok = pngi_symbol(br, S.lcount, S.lsym, 288) == 256;
                            br.need();
                            ok = ok && br.get(3) == (last_seg ? 1u : 0u);
                            br.skip((int)((8 - (br.pos() & 7)) & 7));
                            br.need();
                            ok = ok && br.peek(32) == 0xffff0000u;
                            br.skip(32);
                            ok = ok && br.pos() == base_bit + chunk_bits - (last_seg ? 32 : 0);
                            if (!ok) err |= PI_ERR_TRAILER;
                        }
                    }
                }
                pngi_zero(S, i, end);            // what an error leaves undecoded: zeros, nothing pending there
                if (err) PNGI_OR(&S.status, err);
                if (pend) S.pending = 1;
            }
        }
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            for (int w = 0; w < PI_WORDS; w++) S.written[tid * PI_WORDS + w] = S.fresh[tid * PI_WORDS + w];
        }
        // rounds
        for (int round = 0; round < nsub; round++) {
            PNGI_SYNC();
            const int pending = S.pending;
            PNGI_SYNC();
            if (!pending) break;
            PNGI_EACH_THREAD(tid, PI_THREADS) {
                if (tid == 0) { S.pending = 0; S.progress = 0; }
            }
            PNGI_EACH_THREAD(tid, PI_THREADS) {
                const int start = tid * PI_SUB, end = start + PI_SUB;           // (bits behind n are set)
                int i = start, pend = 0, prog = 0;
                while (i < end) {
                    const uint32_t open = ~S.fresh[i >> 5] >> (i & 31);
                    if (open == 0u) { i = ((i >> 5) + 1) << 5; continue; }
                    i += __builtin_ctz(open);
                    if (i + 3 > end) break;                                     // (cannot happen: a parked match is three bytes at least)
                    const unsigned rec = (unsigned)S.out[i] | ((unsigned)S.out[i + 1] << 8) | ((unsigned)S.out[i + 2] << 16);
                    int len = 3 + (int)(rec >> 15), dist = 1 + (int)(rec & 0x7fffu);
                    if (len > end - i) len = end - i;
                    if (dist > i) dist = i;                                     // (parked matches passed both tests)
                    if (dist >= 1 && pngi_try_copy(S, start, i, len, dist)) prog = 1; else pend = 1;
                    i += len;
                }
                if (pend) S.pending = 1;
                if (prog) S.progress = 1;
            }
            PNGI_EACH_THREAD(tid, PI_THREADS) {
                for (int w = 0; w < PI_WORDS; w++) S.written[tid * PI_WORDS + w] = S.fresh[tid * PI_WORDS + w];
            }
            PNGI_SYNC();
            const int progress = S.progress;
            PNGI_SYNC();
            if (!progress) break;
        }
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            if (tid == 0 && S.pending) S.status |= PI_ERR_STUCK;
        }
    }
    // the filter bytes inside this segment against the index
    const long stride = 1 + 3L * p.W;
    PNGI_EACH_THREAD(tid, PI_THREADS) {
        int err = 0;
        for (long y = (first + stride - 1) / stride + tid; y < p.H && y * stride < first + n; y += PI_THREADS)
            if (S.out[y * stride - first] != p.files[pngi_clampl(f0 + ix + 12 + y, f0, f1 - 1)]) err = PI_ERR_FILTER;
        if (err) PNGI_OR(&S.status, err);
    }
    // out: aligned dwords, the bytes at the two ends singly
    const long dst0 = page * p.total + first;
    if (dst0 >= 0 && dst0 + n <= p.stream_bytes) {
        PNGI_EACH_THREAD(tid, PI_THREADS) {
            const int head = (int)((4 - (dst0 & 3)) & 3) < n ? (int)((4 - (dst0 & 3)) & 3) : n;
            const int body = (n - head) >> 2, tail0 = head + 4 * body;
            uint32_t* dw = reinterpret_cast<uint32_t*>(p.stream + dst0 + head);
            for (int k = tid; k < body; k += PI_THREADS) {
                const uint8_t* b = S.out + head + 4 * k;
                dw[k] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
            }
            for (int k = tid; k < head + (n - tail0); k += PI_THREADS) {
                const int b = k < head ? k : tail0 + (k - head);
                p.stream[dst0 + b] = S.out[b];
            }
        }
    }
    PNGI_EACH_THREAD(tid, PI_THREADS) {
        if (tid == 0 && S.status) p.status[page] = S.status;
    }
}

}  // namespace ldetr
