// Stand-alone check of egotap_amd/csrc/lds_opt_in.h (tests/test_lds_opt_in_cpu.py builds and runs it, plain and with -fsanitize=thread):
// 8 threads ask for every pair of 16 fake kernel addresses x 4 device ordinals, each in its own order, several times over.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "lds_opt_in.h"

static constexpr int THREADS = 8, KERNELS = 16, DEVICES = 4, ROUNDS = 5, PAIRS = KERNELS * DEVICES;
static char g_kernels[KERNELS];             // their addresses stand for kernel handles
static LdsOptIn g_seen;
static std::atomic<int> g_calls[PAIRS];     // how often a pair was told "make the HIP call"
static int g_granted[PAIRS];                // written inside `set` only: the table's lock is what orders these writes
static std::atomic<int> g_fail{0};

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);   \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

static int ask(int pair, int bytes) {
    return g_seen.ensure(&g_kernels[pair / DEVICES], pair % DEVICES, bytes, [pair](int b) {
        ++g_calls[pair];
        g_granted[pair] = b;
        return 0;
    });
}

template <class F>
static void on_threads(F&& body) {
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t) th.emplace_back(body, t);
    for (auto& x : th) x.join();
}

int main() {
    // every pair, a different order per thread (stride coprime to 64, own start), ROUNDS times
    on_threads([](int t) {
        const int stride = 2 * t + 1, start = 7 * t;
        for (int r = 0; r < ROUNDS; ++r)
            for (int i = 0; i < PAIRS; ++i) CHECK(ask((start + i * stride) % PAIRS, 100 * 1024) == 0);
    });
    for (int p = 0; p < PAIRS; ++p) CHECK(g_calls[p] == 1 && g_granted[p] == 100 * 1024);

    // one pair asks for more: one more call, whoever comes first; smaller and equal requests make none
    const int grown = 37;
    on_threads([](int t) {
        for (int r = 0; r < ROUNDS; ++r) {
            CHECK(ask(grown, t % 2 ? 160 * 1024 : 64 * 1024) == 0);
            CHECK(ask((grown + 1 + t) % PAIRS, 100 * 1024 - t) == 0);
        }
    });
    for (int p = 0; p < PAIRS; ++p) CHECK(g_calls[p] == (p == grown ? 2 : 1));
    CHECK(g_granted[grown] == 160 * 1024);

    // a failed call is reported and not recorded: the next request makes the call again
    int tries = 0;
    auto failing = [&tries](int) { ++tries; return 719; };
    CHECK(g_seen.ensure(&g_kernels[0], DEVICES, 1024, failing) == 719);
    CHECK(g_seen.ensure(&g_kernels[0], DEVICES, 1024, failing) == 719 && tries == 2);

    if (g_fail) return 1;
    std::printf("lds_opt_in: %d pairs, %d threads: ok\n", PAIRS, THREADS);
    return 0;
}
