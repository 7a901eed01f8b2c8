// Stand-alone driver for the host side of the streaming resampler (masr_amd/csrc/resample.cpp: masr_resample_rate_fill,
// masr_resample_tile_span, masr_resample_plan) under AddressSanitizer + UBSan.  No GPU, no HIP runtime:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/resample_plan_fuzz.cpp masr_amd/csrc/resample.cpp -o resample_plan_fuzz && ./resample_plan_fuzz
// A few hundred random feed sets: valid ones must be accepted and tiled exactly (every output of every feed in one tile, tiles in
// feed order, the list written into a buffer of exactly the counted size), sets with one broken feed must be refused naming it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "masr_hip.h"

#define REQUIRE(c)                                                      \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "line %d: %s (set %d)\n", __LINE__, #c, set_no); \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    std::mt19937_64 rng(20240817);
    auto uni = [&](long lo, long hi) { return (long)(lo + (long)(rng() % (unsigned long)(hi - lo + 1))); };
    const int src_rates[] = {8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000, 4000};
    static double fake_table[4];                       // (only its address is recorded)
    int set_no = 0, refused = 0, accepted = 0;
    for (set_no = 0; set_no < 600; ++set_no) {
        std::vector<masr_resample_rate> rates;
        const int n_rates = (int)uni(1, 5);
        for (int j = 0; j < n_rates; ++j) {
            masr_resample_rate r;
            const double ratio = 16000.0 / (double)src_rates[uni(0, 8)];
            REQUIRE(masr_resample_rate_fill(ratio, fake_table, 32769, 512, &r) == 0);
            REQUIRE(masr_resample_tile_span(&r) > 0);
            rates.push_back(r);
        }
        masr_resample_rate bad_rate;
        REQUIRE(masr_resample_rate_fill(0.0, fake_table, 32769, 512, &bad_rate) != 0);
        REQUIRE(masr_resample_rate_fill(1.0 / 1024.0, fake_table, 32769, 512, &bad_rate) != 0);
        const int n_feeds = (int)uni(0, 200), dst_rows = (int)uni(1, 64);
        std::vector<masr_resample_feed> feeds;
        std::vector<long> row_at(dst_rows, 0);
        long src_at = 0;
        for (int k = 0; k < n_feeds; ++k) {
            masr_resample_feed f;
            f.rate_slot = (int32_t)uni(0, n_rates - 1);
            f.format = (int32_t)uni(0, 1);
            const double ratio = rates[f.rate_slot].ratio;
            long n_in = uni(1, 3) == 1 ? uni(1, 40) : uni(1, 40000);
            while ((long)((double)n_in * ratio) < 1) ++n_in;
            f.n_in = (int32_t)n_in;
            f.n_out = (int32_t)((double)n_in * ratio);
            src_at += uni(0, 3) * 2;
            if (f.format) src_at = (src_at + 3) & ~3L;
            f.src_offset = src_at;
            src_at += n_in * (f.format ? 4 : 2);
            f.dst_row = (int32_t)uni(0, dst_rows - 1);
            row_at[f.dst_row] += uni(0, 7);
            f.dst_offset = (int32_t)row_at[f.dst_row];
            row_at[f.dst_row] += f.n_out;
            feeds.push_back(f);
        }
        long dst_stride = 1;
        for (long v : row_at) dst_stride = v > dst_stride ? v : dst_stride;
        int64_t n_tiles = -1;
        int32_t bad = 0;
        const char* why = nullptr;
        REQUIRE(masr_resample_plan(feeds.data(), n_feeds, rates.data(), n_rates, src_at, dst_rows, dst_stride, nullptr, 0, &n_tiles, &bad,
                                   &why) == 0);
        REQUIRE(bad == -1 && why == nullptr && n_tiles >= n_feeds);
        std::vector<int32_t> tiles((size_t)(2 * n_tiles));             // exactly the counted size: an overrun is ASan's to find
        int64_t again = -1;
        REQUIRE(masr_resample_plan(feeds.data(), n_feeds, rates.data(), n_rates, src_at, dst_rows, dst_stride, tiles.data(), n_tiles, &again,
                                   nullptr, nullptr) == 0);
        REQUIRE(again == n_tiles);
        int64_t at = 0;
        for (int k = 0; k < n_feeds; ++k)
            for (long t0 = 0; t0 < feeds[k].n_out; t0 += MASR_RESAMPLE_TILE, ++at) REQUIRE(tiles[2 * at] == k && tiles[2 * at + 1] == t0);
        REQUIRE(at == n_tiles);
        if (n_tiles > 1) {                                              // a smaller buffer: filled to its capacity, never beyond
            std::vector<int32_t> fewer((size_t)(2 * (n_tiles / 2)));
            REQUIRE(masr_resample_plan(feeds.data(), n_feeds, rates.data(), n_rates, src_at, dst_rows, dst_stride, fewer.data(), n_tiles / 2,
                                       &again, &bad, &why) == 0 && again == n_tiles);
        }
        ++accepted;
        if (n_feeds == 0) continue;
        // break one feed in one way: refused, naming it
        std::vector<masr_resample_feed> broken = feeds;
        const int k = (int)uni(0, n_feeds - 1);
        masr_resample_feed& f = broken[k];
        long bytes = src_at, stride = dst_stride;
        switch (uni(0, 8)) {
            case 0: f.n_out += 1; break;
            case 1: f.n_out -= 1; break;
            case 2: f.rate_slot = n_rates; break;
            case 3: f.rate_slot = -1; break;
            case 4: f.dst_offset = (int32_t)(dst_stride - f.n_out + 1); break;
            case 5: f.dst_row = dst_rows; break;
            case 6: f.src_offset += 1; break;
            case 7: f.format = 2; break;
            default: f.src_offset = bytes - (long)f.n_in * (f.format ? 4 : 2) + 4; break;
        }
        REQUIRE(masr_resample_plan(broken.data(), n_feeds, rates.data(), n_rates, bytes, dst_rows, stride, tiles.data(), n_tiles, &again, &bad,
                                   &why) != 0);
        REQUIRE(bad == k && why != nullptr);
        // a feed cut short of its outputs: the last output would read at or beyond the input
        broken = feeds;
        if (broken[k].n_out > 2 && rates[broken[k].rate_slot].ratio > 1.0) {
            broken[k].n_in = (int32_t)((double)(broken[k].n_out - 1) * rates[broken[k].rate_slot].time_increment);
            if (broken[k].n_in >= 1)
                REQUIRE(masr_resample_plan(broken.data(), n_feeds, rates.data(), n_rates, bytes, dst_rows, stride, nullptr, 0, &again, &bad, &why) != 0 &&
                        bad == k);
        }
        std::vector<masr_resample_rate> bad_rates = rates;
        bad_rates[0].index_step += 1;
        REQUIRE(masr_resample_plan(feeds.data(), n_feeds, bad_rates.data(), n_rates, bytes, dst_rows, stride, nullptr, 0, &again, &bad, &why) != 0 &&
                bad == -1);
        ++refused;
    }
    std::printf("resample_plan_fuzz: %d feed sets accepted and tiled, %d broken sets refused\n", accepted, refused);
    return 0;
}
