// The body of png_inflate_kernel run on the host, one segment after the other, a phase being a loop over the lane index (csrc/png_inflate_kernel.hpp).
// Meant to be built with the sanitizers and fed corrupted files, which never go to a GPU (tests/test_png_inflate_cpu.py):
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o png_inflate_hostcheck tools/png_inflate_hostcheck.cpp
//     png_inflate_hostcheck JOB
// JOB (little-endian int64 words, then bytes): 'LDIXJOB1', H, W, segments, file bytes, offset of the ldIX data in the file; the segment table
// [segments][4] = (offset of the IDAT data, bytes, kind, first index entry); the file; the H (1 + 3 W) bytes of filtered stream the file must give.
// Prints the status word.  Exit code 0: status 0 and the stream reproduced byte for byte; 3: a non-zero status; 4: status 0 but another stream; 2: bad job.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../layoutdetr_amd/csrc/png_inflate_kernel.hpp"

using namespace ldetr;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s JOB\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t head[6];
    if (fread(head, 8, 6, f) != 6 || memcmp(head, "LDIXJOB1", 8) != 0) { fprintf(stderr, "not a job file\n"); return 2; }
    const int64_t H = head[1], W = head[2], nseg = head[3], file_bytes = head[4], index_off = head[5];
    if (H < 1 || W < 1 || H > 32768 || W > 4096 || file_bytes < 1 || file_bytes > (1LL << 30)) { fprintf(stderr, "bad job header\n"); return 2; }
    const int64_t total = H * (1 + 3 * W);
    if (nseg != (total + PI_SEG - 1) / PI_SEG) { fprintf(stderr, "bad segment count\n"); return 2; }
    std::vector<int64_t> seg(4 * nseg);
    const int64_t padded = (file_bytes + 15) / 16 * 16;
    // exactly the padded size, on the heap: the sanitizer sees every byte the kernel may touch and not one more
    uint8_t* files = static_cast<uint8_t*>(aligned_alloc(16, (size_t)padded));
    uint8_t* stream = static_cast<uint8_t*>(aligned_alloc(16, (size_t)((total + 15) / 16 * 16)));
    std::vector<uint8_t> want(total);
    memset(files, 0, (size_t)padded);
    memset(stream, 0xa5, (size_t)((total + 15) / 16 * 16));
    if (fread(seg.data(), 8, seg.size(), f) != seg.size() || fread(files, 1, (size_t)file_bytes, f) != (size_t)file_bytes || fread(want.data(), 1, (size_t)total, f) != (size_t)total) {
        fprintf(stderr, "truncated job file\n");
        return 2;
    }
    fclose(f);
    const int64_t file_off[2] = {0, file_bytes};
    int32_t status = 0;
    PngInflateParams p;
    p.files = files; p.files_bytes = padded; p.file_off = file_off; p.seg = seg.data(); p.index_off = &index_off;
    p.stream = stream; p.stream_bytes = (total + 15) / 16 * 16; p.status = &status; p.n = 1; p.H = (int)H; p.W = (int)W; p.nseg = nseg; p.total = total;
    PngInflateShared* S = new PngInflateShared;
    for (int64_t s = 0; s < nseg; s++) {
        memset(S, 0xcd, sizeof(*S));                   // LDS is not zero when a workgroup starts
        png_inflate_segment(*S, p, 0, s);
    }
    delete S;
    const bool same = memcmp(stream, want.data(), (size_t)total) == 0;
    printf("status %d stream %s\n", status, same ? "equal" : "differs");
    free(files); free(stream);
    return status ? 3 : (same ? 0 : 4);
}
