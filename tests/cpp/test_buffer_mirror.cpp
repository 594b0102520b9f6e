// test_buffer_mirror.cpp -- the file calls of the C++ host mirror (foo-dsp-bfir_amd/host/buffer_hip.hpp, coeff_hip.hpp,
// brutefir_hip.hpp), used the way the plug-in uses them for an impulse file (foo_dsp_bfir.cpp:181-233): check_snd_file, and
// where the file's rate is not the stream's, resample_snd_file and set_coeff on the cached file.  The impulse and the audio
// come from integer recurrences that tests/test_resample_gpu.py restates; the FNV-1a hash of the output bytes is printed
// for it.  argv[1]: a directory to work in.
// Build: g++ -std=c++17 tests/cpp/test_buffer_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../foo-dsp-bfir_amd/host/brutefir_hip.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } \
    } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s <directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1], file = dir + "/impulse.wav";
    const int L = 256, B = 6, C = 2, nb = 8, n_ir = 1500, file_rate = 44100, rate = 48000;

    std::vector<float> ir((size_t)n_ir * C);
    for (int n = 0; n < n_ir; n++)
        for (int c = 0; c < C; c++) {
            const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(c + 3))) & 0xffffu;
            ir[(size_t)n * C + c] = (float)(((double)k / 65536.0 - 0.5) / (8.0 * (1.0 + (double)n / 64.0)));
        }
    buffer::save_to_snd_file(file.c_str(), ir.data(), C, n_ir, 4, file_rate);

    int ch = 0, frames = 0, sr = 0;
    CHECK(buffer::get_snd_file_params(file.c_str(), &ch, &frames, &sr) && ch == C && frames == n_ir && sr == file_rate, "params");
    CHECK(!buffer::get_snd_file_params((dir + "/absent.wav").c_str(), &ch, &frames, &sr), "an absent file");
    CHECK(buffer::check_snd_file(file.c_str(), C, file_rate) && !buffer::check_snd_file(file.c_str(), C, rate) &&
              !buffer::check_snd_file(file.c_str(), 3, file_rate), "check_snd_file");

    // load_from_snd_file: max_frames and pad (buffer.cpp:60-71); deinterlace / interlace
    int n_ch = 0, n_fr = 0;
    double *d = (double *)buffer::load_from_snd_file(file.c_str(), &n_ch, &n_fr, 8, 2000, true);
    CHECK(d && n_ch == C && n_fr == n_ir && d[5] == (double)ir[5] && d[(size_t)1999 * C + 1] == 0.0, "load, padded");
    void **parts = buffer::deinterlace(d, C, 2000, 8);
    double *again = (double *)buffer::interlace(parts, C, 2000, 8);
    CHECK(memcmp(again, d, sizeof(double) * 2000 * C) == 0 && ((double *)parts[1])[7] == d[7 * C + 1], "interlace(deinterlace(x)) is x");
    for (int c = 0; c < C; c++) bfir_aligned_free(parts[c]);
    bfir_aligned_free(parts); bfir_aligned_free(again); bfir_aligned_free(d);
    float *fl = (float *)buffer::load_from_snd_file(file.c_str(), &n_ch, &n_fr, 4, 100, false);
    CHECK(fl && n_fr == 100 && fl[199] == ir[199], "load, cut");
    bfir_aligned_free(fl);
    int length = 0, n_coeffs = 0;
    void **co = coeff::load_snd_coeff(file.c_str(), &length, 4, 300, &n_coeffs);
    CHECK(co && length == 300 && n_coeffs == C && ((float *)co[1])[299] == ir[(size_t)299 * C + 1], "load_snd_coeff");
    for (int c = 0; c < n_coeffs; c++) bfir_aligned_free(co[c]);
    bfir_aligned_free(co);

    brutefir filter(L, B, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE, rate, false);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(filter.set_coeff(file.c_str(), B, 0.5) == -1 && !filter.is_initialized(), "a file at another rate is incompatible");
    CHECK(filter.set_coeff((dir + "/absent.wav").c_str(), B, 0.5) == -1, "an absent file is incompatible");
    CHECK(buffer::resample_snd_file(file.c_str(), 3, rate, dir).empty(), "fewer channels than asked");
    const std::string cached = buffer::resample_snd_file(file.c_str(), C, rate, dir);
    CHECK(cached == dir + "/" + buffer::cache_name(file.c_str(), C, rate), "cache name: %s", cached.c_str());
    CHECK(buffer::get_snd_file_params(cached.c_str(), &ch, &frames, &sr) && ch == C && sr == rate &&
              frames == (int)(((int64_t)n_ir * 160 + 146) / 147), "the cached file: %d frames", frames);
    CHECK(buffer::resample_snd_file(file.c_str(), C, rate, dir) == cached, "the cached file is reused");
    printf("cached %s\n", cached.c_str());
    CHECK(filter.set_coeff(cached.c_str(), B, 0.5) == C && filter.is_initialized(), "set_coeff(filename)");
    const std::wstring wide(cached.begin(), cached.end());
    CHECK(filter.set_coeff(wide.c_str(), B, 0.5) == C, "set_coeff(wide filename)");

    std::vector<float> x((size_t)nb * L * C), y(x.size());
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    for (int t = 0; t < nb; t++)
        CHECK(filter.run(&x[(size_t)t * L * C], &y[(size_t)t * L * C]) == 0, "run block %d", t);
    uint64_t hash = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)y.data();
    for (size_t i = 0; i < y.size() * sizeof(float); i++) hash = (hash ^ p[i]) * 0x100000001b3ull;
    printf("checksum %016llx\n", (unsigned long long)hash);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
