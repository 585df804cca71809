// strip_probe.cpp — the line stripper's input rate on one core and on T
// threads (sid_strip_lines_impl, strip.cpp), over synthetic 30x lines of about
// 81 B (or --depth D).  CPU only; prints one JSON line.
//   c++ -O2 -std=c++17 -Iinclude -Isid_amd/csrc tools/debug/strip_probe.cpp sid_amd/csrc/strip.cpp -lpthread
//   strip_probe [--mib 256] [--depth 30] [--threads 1] [--reps 5]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "strip.h"

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv)
{
    size_t mib = 256;
    int depth = 30, threads = 1, reps = 5;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!std::strcmp(argv[i], "--mib")) mib = std::strtoull(argv[i + 1], nullptr, 10);
        else if (!std::strcmp(argv[i], "--depth")) depth = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--threads")) threads = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--reps")) reps = std::atoi(argv[i + 1]);
    }
    const size_t want = mib << 20;
    std::string text;
    text.reserve(want + 4096);
    uint64_t x = 88172645463325252ull, site = 0;
    auto rnd = [&] { x ^= x << 13, x ^= x >> 7, x ^= x << 17; return x; };
    while (text.size() < want) {
        ++site;
        const int d = depth - 3 + (int)(rnd() % 7);
        text += "chr" + std::to_string(1 + site / 4000000) + "\t" + std::to_string(site % 4000000 + 1) + "\tA\t" +
                std::to_string(d) + "\t";
        for (int r = 0; r < d; ++r) {
            const uint64_t v = rnd() % 100;
            if (v < 2) text += "^]";
            text += v < 48 ? '.' : v < 96 ? ',' : "ACGT"[v & 3];
            if (v > 97) text += '$';
        }
        text += '\t';
        for (int r = 0; r < d; ++r) text += (char)('!' + rnd() % 40);
        text += '\n';
    }
    const size_t n = text.size();
    std::vector<char> out(n + 64 * (size_t)threads), ref(n);
    uint64_t lines = 0;
    const size_t m0 = sid_strip_lines_impl(SID_STRIP_SCALAR, text.data(), n, ref.data(), n, &lines);
    std::printf("{\"bytes\": %zu, \"lines\": %llu, \"bytes_per_line\": %.1f, \"stripped_per_line\": %.1f, \"auto\": %d, "
                "\"threads\": %d",
                n, (unsigned long long)lines, (double)n / lines, (double)m0 / lines, sid_strip_impl(), threads);
    static const char* NAME[] = {"", "scalar", "avx2", "avx512"};
    for (int impl = 1; impl <= 3; ++impl) {
        if (sid_strip_lines_impl(impl, text.data(), 0, out.data(), 0, nullptr) == (size_t)-1) continue;
        double best = 1e30;
        bool same = true;
        for (int rep = 0; rep < reps; ++rep) {
            // thread t: a line-aligned T-th of the text into its own part of out
            std::vector<size_t> cut(threads + 1, n);
            cut[0] = 0;
            for (int t = 1; t < threads; ++t) {
                const char* nl = (const char*)std::memchr(text.data() + n * t / threads, '\n', n - n * t / threads);
                cut[t] = nl ? (size_t)(nl - text.data()) + 1 : n;
            }
            std::vector<size_t> got(threads, 0);
            const double t0 = now();
            std::vector<std::thread> th;
            for (int t = 0; t < threads; ++t)
                th.emplace_back([&, t] {
                    got[t] = sid_strip_lines_impl(impl, text.data() + cut[t], cut[t + 1] - cut[t], out.data() + cut[t],
                                                  cut[t + 1] - cut[t], nullptr);
                });
            for (auto& h : th) h.join();
            best = std::min(best, now() - t0);
            size_t at = 0;
            for (int t = 0; t < threads; ++t) {
                same = same && at + got[t] <= m0 && !std::memcmp(out.data() + cut[t], ref.data() + at, got[t]);
                at += got[t];
            }
            same = same && at == m0;
        }
        std::printf(", \"%s\": {\"GBps_in\": %.2f, \"equal_to_scalar\": %s}", NAME[impl], n / best / 1e9,
                    same ? "true" : "false");
    }
    std::printf("}\n");
    return 0;
}
