// jpeg_entropy_sweep.cpp -- the host entropy stage (styl3r_amd/csrc/gsr_jpeg_entropy.h) alone, for the host sanitizers: the header has
// no HIP include and this file is a plain C++17 program.  For every JPEG file on the command line it decodes
//   * the stream itself (must be GSR_OK),
//   * every proper prefix of it,
//   * the stream with each single byte of its first 700 set to 0x00 and to 0xFF,
// each copied into a heap block of EXACTLY its length (so that AddressSanitizer sees a read one byte past the stream), into a
// coefficient buffer of exactly the size gsr_jpeg_coef_bytes would report, and probes it as well.  Every call must answer with one of
// the three statuses.  Exit code 0 and "clean" when nothing else happened.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_entropy_sweep.cpp -o sweep
//   python -c "import numpy as np; z = np.load('tests/golden/jpeg_frames.npz'); [z[k].tofile(k + '.jpg') for k in z.files if k.startswith('jpg_')]"
//   ./sweep jpg_*.jpg
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../styl3r_amd/csrc/gsr_jpeg_entropy.h"

static long g_calls = 0, g_status[3] = {0, 0, 0};

// one stream in a heap block of exactly its length -> status; aborts the program on an answer outside the three statuses
static int run(const std::vector<uint8_t> &bytes, int H, int W)
{
    std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes.size() ? bytes.size() : 1]);
    if (!bytes.empty()) memcpy(exact.get(), bytes.data(), bytes.size());
    const uint8_t *data = exact.get();
    const size_t len = bytes.size();
    gsr_jpeg_info info;
    const int pr = gsr_jpeg::probe(data, len, &info);
    std::vector<int16_t> coefs((size_t)gsr_jpeg::max_image_coefs(H, W));
    gsr_jpeg_desc desc;
    int32_t status = -7;
    const int rc = gsr_jpeg::entropy(&data, &len, 1, H, W, coefs.data(), &desc, &status, 1);
    ++g_calls;
    if (rc != GSR_OK || status < 0 || status > 2 || pr < 0 || pr > 2 || (status == GSR_OK && pr != GSR_OK) ||
        desc.coef_count != (status == GSR_OK ? desc.coef_count : 0) || desc.coef_count > (int64_t)coefs.size()) {
        fprintf(stderr, "bad answer: rc %d status %d probe %d count %lld\n", rc, status, pr, (long long)desc.coef_count);
        exit(2);
    }
    ++g_status[status];
    return status;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]);
        return 1;
    }
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        const std::vector<uint8_t> base((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        gsr_jpeg_info info;
        const int pr = gsr_jpeg::probe(base.data(), base.size(), &info);
        if (pr != GSR_OK) {   // the fallback streams: swept at the size their frame header gives, if it gives one
            info.width = info.width > 0 ? info.width : 8;
            info.height = info.height > 0 ? info.height : 8;
        }
        const int H = info.height, W = info.width;
        const int whole = run(base, H, W);
        if (pr == GSR_OK && whole != GSR_OK && std::string(argv[a]).find("truncated") == std::string::npos) {
            fprintf(stderr, "%s: a fast-path stream did not decode (%d)\n", argv[a], whole);
            return 2;
        }
        for (size_t k = 0; k < base.size(); ++k) run(std::vector<uint8_t>(base.begin(), base.begin() + (long)k), H, W);
        for (size_t k = 0; k < base.size() && k < 700; ++k) {
            for (int v : {0x00, 0xFF}) {
                if (base[k] == v) continue;
                std::vector<uint8_t> m(base);
                m[k] = (uint8_t)v;
                run(m, H, W);
            }
        }
    }
    // several threads over one batch: the workers share nothing but the job counter
    {
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> base((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        gsr_jpeg_info info;
        if (gsr_jpeg::probe(base.data(), base.size(), &info) == GSR_OK) {
            const int64_t N = 24;
            std::vector<const uint8_t *> data((size_t)N, base.data());
            std::vector<size_t> len((size_t)N, base.size());
            for (int64_t n = 0; n < N; n += 3) len[(size_t)n] = base.size() / 2;
            std::vector<int16_t> coefs((size_t)(N * gsr_jpeg::max_image_coefs(info.height, info.width)));
            std::vector<gsr_jpeg_desc> desc((size_t)N);
            std::vector<int32_t> status((size_t)N, -7);
            if (gsr_jpeg::entropy(data.data(), len.data(), N, info.height, info.width, coefs.data(), desc.data(), status.data(), 8) != GSR_OK) return 2;
            for (int64_t n = 0; n < N; ++n)
                if (status[(size_t)n] != (n % 3 == 0 ? GSR_JPEG_CORRUPT : GSR_OK)) {
                    fprintf(stderr, "threaded batch: image %lld has status %d\n", (long long)n, status[(size_t)n]);
                    return 2;
                }
        }
    }
    printf("clean: %ld streams decoded (%ld ok, %ld unsupported, %ld corrupt) from %d files\n", g_calls, g_status[0], g_status[1], g_status[2], argc - 1);
    return 0;
}
