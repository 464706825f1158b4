// png_batch_tsan -- kbn_png_decode_batch (csrc/io_png.hip alone) in a ThreadSanitizer build: 64 inputs, the fixtures and mutants of
// them from codec_fuzz's generator, at least half of them refused, on 1, 2, 8 and 16 threads, with and without a status array.
// Statuses and pixels equal what kbn_png_decode gives one by one, and ThreadSanitizer reports nothing (a report ends the program).
// usage: png_batch_tsan PNG...
#include <memory>

#include "fuzz_common.h"

int main(int argc, char** argv) {
    g_program = "png_batch_tsan";
    setvbuf(stdout, nullptr, _IOLBF, 0);
    __sanitizer_set_death_callback(on_death);
    std::vector<Bytes> fixtures;
    for (int i = 1; i < argc; ++i) fixtures.push_back(read_file(argv[i]));
    REQUIRE(!fixtures.empty(), "no fixture given");
    g_seed = 77;
    Rng r(g_seed);
    constexpr int N = 64;
    g_stage = "one by one";
    // inputs: kept when they fill the quota of their kind (accepted / refused), so that each half is there
    std::vector<Bytes> files;
    std::vector<int> want_status;
    std::vector<Bytes> want_pixels;
    int accepted = 0, refused = 0;
    for (long long tries = 0; (int)files.size() < N; ++tries) {
        g_iteration = tries;
        REQUIRE(tries < 100000, "the generator does not fill both halves");
        const Bytes& base = fixtures[r.below((uint32_t)fixtures.size())];
        Bytes f;
        switch (r.below(4)) {
            case 0: f = base; break;
            case 1: f = png_mutate_bytes(base, r); break;
            default: f = png_mutate_deep(png_parse(base), (int)r.below(PNG_DEEP_KINDS), (int)r.below(8), r); break;
        }
        int w = 0, h = 0, c = 0, depth = 0;
        const bool informed = kbn_png_info(f.data(), f.size(), &w, &h, &c, &depth) == KBN_OK;
        const unsigned long long need = informed ? (unsigned long long)w * h * c * (depth / 8) : 0;
        if (need > (1ull << 22)) continue;
        size_t size = informed ? (size_t)need : 64;
        if (informed && r.below(8) == 0) size -= 1;               // refused for its pixels_bytes
        Bytes pixels(size, 0xA5);
        const int rc = kbn_png_decode(f.data(), f.size(), pixels.data(), pixels.size());
        if (rc == KBN_OK ? accepted >= N / 2 : refused >= N / 2) continue;
        ++(rc == KBN_OK ? accepted : refused);
        files.push_back(f);
        want_status.push_back(rc);
        want_pixels.push_back(pixels);
    }
    int first_failure = KBN_OK;
    for (int i = N - 1; i >= 0; --i)
        if (want_status[i] != KBN_OK) first_failure = want_status[i];
    long long batches = 0;
    for (int threads : {1, 2, 8, 16})
        for (int with_status = 0; with_status < 2; ++with_status)
            for (int repeat = 0; repeat < 3; ++repeat) {
                g_stage = "batch";
                g_iteration = 100 * threads + 10 * with_status + repeat;
                std::vector<std::unique_ptr<Block>> in, out;
                std::vector<const unsigned char*> file_ptr;
                std::vector<size_t> file_bytes, pixel_bytes;
                std::vector<void*> pixel_ptr;
                for (int i = 0; i < N; ++i) {
                    in.emplace_back(new Block(files[i]));
                    out.emplace_back(new Block(want_pixels[i].size()));
                    file_ptr.push_back(in[i]->p); file_bytes.push_back(in[i]->n);
                    pixel_ptr.push_back(out[i]->p); pixel_bytes.push_back(out[i]->n);
                }
                std::vector<int> status(N, 12345);
                const int rc = kbn_png_decode_batch(file_ptr.data(), file_bytes.data(), pixel_ptr.data(), pixel_bytes.data(), N, threads, with_status ? status.data() : nullptr);
                REQUIRE(rc == first_failure, "%d threads: the batch answers %d, the first failure one by one is %d", threads, rc, first_failure);
                for (int i = 0; i < N; ++i) {
                    if (with_status) REQUIRE(status[i] == want_status[i], "%d threads: status[%d] = %d, one by one %d", threads, i, status[i], want_status[i]);
                    REQUIRE(memcmp(out[i]->p, want_pixels[i].data(), out[i]->n) == 0, "%d threads: the pixels of input %d differ from kbn_png_decode's", threads, i);
                }
                ++batches;
            }
    printf("png_batch_tsan: %d inputs (%d decoded, %d refused), %lld batches on 1, 2, 8 and 16 threads\n", N, accepted, refused, batches);
    printf("png_batch_tsan: ok\n");
    return 0;
}
