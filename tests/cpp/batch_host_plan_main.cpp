// batch_host_plan_main.cpp -- the planner of dxtlt_transform_batch_host (csrc/batch_host_plan.h: a pure function over the item
// lengths and the chunk cap) as a stand-alone program for the host sanitizers: tests/test_batch_host_plan_sanitized.py builds it
// with -fsanitize=address,undefined and runs it.  It plans every list of up to 4 items drawn from the lengths at which the rule
// turns (tests/test_batch_host_plan.py: the same lists) at two caps, no item at all, and lengths near 2^40, and holds every plan
// to the properties the call relies on.  No device is touched.  Prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "../../dxt-lossless-transform_amd/csrc/batch_host_plan.h"

using namespace dxtlt_host;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

// which items go out alone, slots side by side in the call's order, the chunk bound and the arena bound
static int check_plan(const std::vector<uint64_t>& len, uint64_t cap)
{
    const HostBatchPlan plan = plan_host_batch(len.data(), len.size(), cap);
    CHECK(plan.chunk_of_item.size() == len.size() && plan.slot.size() == len.size());
    size_t k = 0;
    uint64_t largest = 0;
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const HostBatchChunk& ch = plan.chunks[c];
        CHECK(ch.first == k && ch.count >= 1 && ch.first + ch.count <= plan.packed.size());
        uint64_t at = 0;
        size_t non_empty = 0;
        for (; k < ch.first + ch.count; ++k) {
            const size_t i = plan.packed[k];
            CHECK(i < len.size() && (k == 0 || plan.packed[k - 1] < i));
            CHECK(len[i] < 2 * cap && plan.chunk_of_item[i] == c && plan.slot[i] == at && at % 256 == 0);
            at += host_batch_padded(len[i]);
            non_empty += len[i] != 0;
        }
        CHECK(ch.bytes == at && (at <= cap || non_empty == 1));
        // closed BEFORE the item that would have overfilled it, and only because it held bytes
        if (c + 1 < plan.chunks.size())
            CHECK(at > 0 && at + host_batch_padded(len[plan.packed[k]]) > cap);
        largest = at > largest ? at : largest;
    }
    CHECK(k == plan.packed.size() && plan.arena_bytes == largest && (largest < 3 * cap || cap == 0));
    size_t alone = 0;
    for (size_t i = 0; i < len.size(); ++i) {
        CHECK((plan.chunk_of_item[i] == kHostBatchAlone) == (len[i] >= 2 * cap));
        if (plan.chunk_of_item[i] == kHostBatchAlone) {
            CHECK(plan.slot[i] == 0);
            ++alone;
        }
    }
    CHECK(alone + plan.packed.size() == len.size() && plan.chunks.empty() == plan.packed.empty());
    return 0;
}

static int check_every_short_list(const std::vector<uint64_t>& values, uint64_t cap)
{
    const size_t v = values.size();
    size_t lists = 1;
    for (size_t n = 0; n <= 4; ++n, lists *= v)
        for (size_t code = 0; code < lists; ++code) {
            std::vector<uint64_t> len;
            for (size_t d = 0, rest = code; d < n; ++d, rest /= v)
                len.push_back(values[rest % v]);
            if (check_plan(len, cap) != 0) {
                std::fprintf(stderr, "cap %llu, list %zu of length %zu\n", (unsigned long long)cap, code, n);
                return 1;
            }
        }
    return 0;
}

int main()
{
    for (const uint64_t cap : {uint64_t(1) << 10, uint64_t(1) << 20})
        CHECK(check_every_short_list({0, 1, 255, 256, 257, cap - 256, cap - 255, cap, cap + 1, 2 * cap - 1, 2 * cap, 2 * cap + 1}, cap) == 0);
    // the sums of lengths near 2^40 pass 2^32 and stay far from 2^64
    const uint64_t big = uint64_t(1) << 40;
    CHECK(check_every_short_list({0, 255, big - 257, big - 1, big, big + 1, 2 * big - 1, 2 * big, 3 * big}, big) == 0);
    CHECK(check_every_short_list({1, big - 256, big, 2 * big - 1}, uint64_t(64) << 20) == 0);
    // no item: the length array is not read
    const HostBatchPlan none = plan_host_batch(nullptr, 0, uint64_t(64) << 20);
    CHECK(none.chunks.empty() && none.packed.empty() && none.chunk_of_item.empty() && none.slot.empty() && none.arena_bytes == 0);
    // only empty items: one chunk without a byte; only items that go out alone: no chunk
    const std::vector<uint64_t> empties(5, 0), alone(3, uint64_t(128) << 20);
    const HostBatchPlan e = plan_host_batch(empties.data(), empties.size(), uint64_t(64) << 20);
    CHECK(e.chunks.size() == 1 && e.chunks[0].count == 5 && e.chunks[0].bytes == 0 && e.arena_bytes == 0);
    const HostBatchPlan a = plan_host_batch(alone.data(), alone.size(), uint64_t(64) << 20);
    CHECK(a.chunks.empty() && a.packed.empty() && a.arena_bytes == 0);
    std::printf("ok\n");
    return 0;
}
