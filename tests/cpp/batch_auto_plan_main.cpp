// batch_auto_plan_main.cpp -- the planner of dxtlt_transform_batch_auto_device (csrc/batch_auto_plan.h: pure host functions) and the
// pieces it shares with the batched pixel auto call (csrc/batch_auto_common.h: the overlap rule, the chunk packer, the section
// table) as a stand-alone program for the host sanitizers: tests/test_batch_auto_plan_sanitized.py builds it with
// -fsanitize=address,undefined and runs it.  It plans the no-device cases of tests/test_batch_auto_plan.py -- every (format,
// use_all) kind at every block count, the 280 000-byte cap with its oversize items, every refusal in both positions, the overlap
// rule both ways, the winners' limit -- and writes the call's tables for a made-up arena address, checked against a statement of
// its own.  No device is touched and no address is dereferenced.  Prints "ok" and returns 0, or says what failed.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../dxt-lossless-transform_amd/csrc/batch_auto_plan.h"

namespace ba = dxtlt_host::batch_auto;
using namespace dxtlt_host;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static void* at(uint64_t a) { return reinterpret_cast<void*>(static_cast<uintptr_t>(a)); }

static DxtltBatchAutoItem item(int format, uint64_t in, uint64_t out, uint64_t len, bool use_all)
{
    DxtltBatchAutoItem it{};
    it.d_input = at(in), it.d_output = at(out), it.len = len;
    it.format = (uint8_t)format, it.use_all_decorrelation_modes = use_all ? 1 : 0;
    return it;
}

static uint64_t block_bytes(int format) { return format == 1 || format == 4 ? 8 : 16; }
static uint64_t windows(uint64_t len) { return (len + 32767) / 32768; }

// the lengths of the sections an item shows the estimator, in slice order (tests/batch_auto_util.py: shown_lengths)
static std::vector<uint64_t> shown_lengths(const DxtltBatchAutoItem& it)
{
    const uint64_t blocks = it.len / block_bytes(it.format);
    const size_t variants = it.use_all_decorrelation_modes && it.format <= 3 ? 4 : 2;
    std::vector<uint64_t> out;
    if (it.format >= 4)
        return std::vector<uint64_t>(it.format == 4 ? 2 : 4, blocks * 2);
    if (it.format == 3)
        out.assign(2, blocks * 2);
    out.insert(out.end(), 2 * variants, blocks * 4);
    return out;
}

// a plan and the tables written from it for an arena at `arena`, against the statement above
static int check_plan_and_tables(const std::vector<DxtltBatchAutoItem>& items, const ba::Plan& plan, uint64_t cap)
{
    uint64_t counter = 0;
    size_t next = 0;
    CHECK(plan.items.size() == items.size());
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const ba::PlannedChunk& ch = plan.chunks[c];
        CHECK(ch.first == next && ch.count >= 1);
        uint64_t off = 0, wgs = 0;
        for (size_t i = ch.first; i < ch.first + ch.count; ++i) {
            const ba::PlannedItem& p = plan.items[i];
            const std::vector<uint64_t> want = shown_lengths(items[i]);
            CHECK(p.chunk == c && p.slice_off == off && p.first_counter == counter && (size_t)p.sections == want.size());
            uint64_t in_slice = 0;
            for (size_t k = 0; k < want.size(); ++k) {
                CHECK(p.sec_off[k] == in_slice && p.sec_len[k] == want[k]);
                in_slice += want[k];
                wgs += windows(want[k]);
            }
            CHECK(p.slice_bytes == in_slice);
            off += (in_slice + 15) & ~uint64_t(15);
            counter += want.size();
        }
        CHECK(ch.arena_bytes == off && ch.estimator_wgs == wgs && (off <= cap || ch.count == 1));
        if (c + 1 < plan.chunks.size())   // closed only when the next item would not fit
            CHECK(off + ((plan.items[ch.first + ch.count].slice_bytes + 15) & ~uint64_t(15)) > cap);
        next += ch.count;
    }
    CHECK(next == items.size() && plan.counters == counter);

    const uint64_t arena_at = 0x3000000000ull;
    std::vector<uint8_t> table(plan.table_bytes + 16);
    uint8_t* host = table.data() + (16 - reinterpret_cast<uintptr_t>(table.data()) % 16) % 16;
    ba::fill_tables(plan, items.data(), static_cast<uint8_t*>(at(arena_at)), host);
    size_t table_at = 0;
    for (const ba::PlannedChunk& ch : plan.chunks) {
        for (int g = 0; g < ba::kGroups; ++g) {   // per launch, the entries in item order
            const dxtlt::BatchAutoEntry* e = reinterpret_cast<const dxtlt::BatchAutoEntry*>(host + ch.at[g]);
            CHECK(ch.at[g] == table_at);
            uint32_t wg = 0, n = 0;
            for (size_t i = ch.first; i < ch.first + ch.count; ++i) {
                const DxtltBatchAutoItem& it = items[i];
                if (it.len == 0 || it.format != g / 2 + 1 || (it.use_all_decorrelation_modes && it.format <= 3) != ((g & 1) != 0))
                    continue;
                const uint64_t blocks = it.len / block_bytes(it.format), lanes = it.format == 1 || it.format == 4 ? (blocks + 1) / 2 : blocks;
                CHECK(n < ch.entries[g] && e[n].src == it.d_input && e[n].arena_off == plan.items[i].slice_off && e[n].blocks == blocks);
                CHECK(e[n].first_wg == wg && e[n].reserved == 0);
                wg += (uint32_t)((lanes + 255) / 256);
                ++n;
            }
            CHECK(n == ch.entries[g] && wg == ch.wgs[g]);
            table_at += n * sizeof(dxtlt::BatchAutoEntry);
        }
        const dxtlt::EstimateTableEntry* s = reinterpret_cast<const dxtlt::EstimateTableEntry*>(host + ch.sections_at);
        CHECK(ch.sections_at == table_at);
        uint32_t end = 0, n = 0;
        for (size_t i = ch.first; i < ch.first + ch.count; ++i) {
            const ba::PlannedItem& p = plan.items[i];
            for (int k = 0; k < p.sections && items[i].len != 0; ++k, ++n) {
                end += (uint32_t)windows(p.sec_len[k]);
                CHECK(n < ch.estimator_entries && s[n].base == at(arena_at + p.slice_off + p.sec_off[k]) && s[n].len == p.sec_len[k]);
                CHECK(s[n].end_wg == end && s[n].counter == p.first_counter + (uint64_t)k);
            }
        }
        CHECK(n == ch.estimator_entries && end == ch.estimator_wgs);
        table_at += (n * sizeof(dxtlt::EstimateTableEntry) + 15) & ~size_t(15);
    }
    CHECK(table_at == plan.table_bytes);
    return 0;
}

static int check_shared_pieces()
{
    // the packer: slices around a 16-byte step and around the cap, in three orders; a counter more per item
    const uint64_t cap = 4096;
    const uint64_t slices[8] = {0, 1, 15, 16, 17, cap - 16, cap, cap + 1};
    for (int order = 0; order < 3; ++order) {
        std::vector<uint64_t> seq(slices, slices + 8);
        if (order == 1)
            std::reverse(seq.begin(), seq.end());
        if (order == 2)
            std::rotate(seq.begin(), seq.begin() + 5, seq.end());
        std::vector<PackedChunk> chunks, one;
        ChunkPacker<PackedChunk> pack{chunks, cap}, whole{one, UINT64_MAX};
        std::vector<PackedItem> items(8), in_one(8);
        for (size_t i = 0; i < 8; ++i) {
            const uint64_t padded = (seq[i] + 15) & ~uint64_t(15);
            const bool closes = !chunks.empty() && chunks.back().arena_bytes + padded > cap;
            const size_t before = chunks.size();
            pack.add(seq[i], (uint32_t)i + 1, items[i]);
            whole.add(seq[i], (uint32_t)i + 1, in_one[i]);
            CHECK(chunks.size() == (before == 0 ? 1 : before + (closes ? 1 : 0)));
            CHECK(items[i].chunk == chunks.size() - 1 && items[i].slice_off % 16 == 0 && items[i].slice_off + padded == chunks.back().arena_bytes);
            CHECK(items[i].first_counter == in_one[i].first_counter && items[i].first_counter == i * (i + 1) / 2);   // whatever the cap
            CHECK(chunks[items[i].chunk].first + chunks[items[i].chunk].count == i + 1);
        }
        CHECK(one.size() == 1 && one[0].count == 8 && pack.counters == 36 && whole.counters == 36);
        uint64_t most = 0;
        for (size_t i = 0; i < 8; ++i) {
            const PackedChunk& c = chunks[items[i].chunk];
            CHECK(c.arena_bytes <= cap || c.count == 1);
            CHECK(seq[i] <= cap || (c.count == 1 && c.arena_bytes == cap + 16));   // an oversize item is alone
            most = std::max(most, c.arena_bytes);
        }
        CHECK(pack.arena_bytes == most && most == cap + 16);
    }

    // the overlap rule: (in, out) of two items of n bytes; inputs may overlap, touching spans do not
    const uint64_t A = 0x100000, B = 0x200000, C = 0x300000, D = 0x400000, n = 256;
    struct Case {
        uint64_t in0, out0, in1, out1;
        bool refused;
    };
    const Case cases[] = {{A, A + n - 1, C, D, true},   // an output over its own input
                          {A, B, B + n - 1, D, true},   // an output over a later input
                          {A, B, C, A + 8, true},       // an output over an earlier input
                          {A, B, C, B + n - 1, true},   // two outputs
                          {A, B, A + 8, D, false},      // two inputs
                          {A, A + n, A + 2 * n, A + 3 * n, false}};   // touching
    for (const Case& k : cases)
        for (int swapped = 0; swapped < 2; ++swapped) {
            OverlapCheck spans;
            spans.add(at(swapped ? k.in1 : k.in0), at(swapped ? k.out1 : k.out0), n);
            spans.add(at(A), at(A), 0);   // an empty item takes no part
            spans.add(at(swapped ? k.in0 : k.in1), at(swapped ? k.out0 : k.out1), n);
            CHECK(spans.spans.size() == 4 && spans.an_output_overlaps() == k.refused);
        }
    return 0;
}

int main()
{
    const uint64_t default_cap = DXTLT_BATCH_AUTO_ARENA_CAP;
    ba::Plan plan, capped;

    // every (format, use_all) kind at every block count, at any alignment
    const uint64_t counts[] = {0, 1, 2, 3, 8191, 8192, 8193};
    std::vector<DxtltBatchAutoItem> items;
    uint64_t where = 0x10000000;
    for (int kind = 0; kind < 8; ++kind)
        for (uint64_t blocks : counts) {
            const int format = kind < 6 ? kind / 2 + 1 : kind - 2;
            items.push_back(item(format, where + 3, where + (1 << 20) + 1, blocks * block_bytes(format), kind < 6 && kind % 2 == 1));
            where += 4 << 20;
        }
    CHECK(ba::plan_call(items.data(), items.size(), default_cap, plan).code == kOk);
    CHECK(plan.chunks.size() == 1 && plan.chunks[0].candidate_launches() == 8 && plan.any);
    CHECK(plan.items[0].sections == 4 && plan.items[7].sections == 8);   // bc1 fast, bc1 all modes: an empty item too
    if (check_plan_and_tables(items, plan, default_cap))
        return 1;
    // the 280 000-byte cap: BC3 with all modes at 8191, 8192 and 8193 blocks (36 bytes per block) alone in their chunks
    const uint64_t cap = 280000;
    CHECK(ba::plan_call(items.data(), items.size(), cap, capped).code == kOk && capped.chunks.size() >= 8);
    if (check_plan_and_tables(items, capped, cap))
        return 1;
    size_t oversize = 0;
    for (size_t i = 0; i < items.size(); ++i) {
        CHECK(capped.items[i].first_counter == plan.items[i].first_counter);   // counters do not depend on the cap
        if (capped.items[i].slice_bytes > cap) {
            CHECK(capped.chunks[capped.items[i].chunk].count == 1);
            ++oversize;
        }
    }
    CHECK(oversize == 3 && capped.arena_bytes == 294960 && capped.counters == plan.counters);

    // an empty call, a NULL array, a batch of empty items
    CHECK(ba::plan_call(items.data(), 0, default_cap, plan).code == kOk && plan.chunks.empty() && !plan.any);
    CHECK(ba::plan_call(nullptr, 3, default_cap, plan).code == kInvalidArgument);
    const DxtltBatchAutoItem empties[2] = {item(1, 0, 0, 0, true), item(5, 0, 0, 0, false)};
    CHECK(ba::plan_call(empties, 2, default_cap, plan).code == kOk && !plan.any && plan.table_bytes == 0 && plan.counters == 12);

    // every refusal, alone, behind and in front of a good item
    const DxtltBatchAutoItem ok = item(1, 0x1000, 0x9000, 64, false);
    struct Bad {
        DxtltBatchAutoItem it;
        int32_t status;
    };
    const Bad bad[] = {{item(1, 0, 0x9000, 64, false), kInvalidArgument},      {item(1, 0x1000, 0, 64, false), kInvalidArgument},
                       {item(0, 0x1000, 0x9000, 64, false), kInvalidArgument}, {item(6, 0x1000, 0x9000, 64, false), kInvalidArgument},
                       {item(7, 0x1000, 0x9000, 64, false), kInvalidArgument}, {item(1, 0x1000, 0x9000, 60, false), kInvalidLength},
                       {item(3, 0x1000, 0x9000, 24, true), kInvalidLength},    {item(1, 0x1000, 0x1020, 64, false), kInvalidArgument}};
    for (const Bad& b : bad) {
        const bool own_input = b.it.d_output == at(0x1020);   // the last: an output over its own input, beside an item elsewhere
        const DxtltBatchAutoItem good = own_input ? item(1, 0x20000, 0x30000, 64, false) : ok;
        const DxtltBatchAutoItem alone[1] = {b.it}, behind[2] = {good, b.it}, front[2] = {b.it, good};
        CHECK(ba::plan_call(alone, 1, default_cap, plan).code == b.status);
        CHECK(ba::plan_call(behind, 2, default_cap, plan).code == b.status);
        CHECK(ba::plan_call(front, 2, default_cap, plan).code == b.status);
    }
    // two overlapping outputs and an output over another item's input, both ways; inputs may overlap; an empty item needs no pointers
    const DxtltBatchAutoItem clash[] = {item(2, 0x2000, 0x9030, 64, false), item(2, 0x2000, 0x1038, 64, false)};
    for (const DxtltBatchAutoItem& c : clash) {
        const DxtltBatchAutoItem ab[2] = {ok, c}, ba_[2] = {c, ok};
        CHECK(ba::plan_call(ab, 2, default_cap, plan).code == kInvalidArgument && ba::plan_call(ba_, 2, default_cap, plan).code == kInvalidArgument);
    }
    const DxtltBatchAutoItem shared[2] = {ok, item(2, 0x1000, 0xA000, 64, false)}, with_empty[2] = {ok, item(2, 0, 0, 0, false)};
    CHECK(ba::plan_call(shared, 2, default_cap, plan).code == kOk && ba::plan_call(with_empty, 2, default_cap, plan).code == kOk);
    // the winners' limit: three BC1 items of 12 GiB are too many tiles for one launch; two are fine, and three of different formats
    std::vector<DxtltBatchAutoItem> big;
    for (uint64_t k = 0; k < 3; ++k)
        big.push_back(item(1, (k + 1) << 40, ((k + 1) << 40) + (16ull << 30), 12ull << 30, false));
    CHECK(ba::plan_call(big.data(), 3, default_cap, plan).code == kInvalidArgument);
    CHECK(ba::plan_call(big.data(), 2, default_cap, plan).code == kOk && plan.chunks.size() == 2);
    big[1].format = 2, big[2].format = 3;
    CHECK(ba::plan_call(big.data(), 3, default_cap, plan).code == kOk);
    const DxtltBatchAutoItem huge = item(1, 1ull << 40, 1ull << 41, 64ull << 30, false);
    CHECK(ba::plan_call(&huge, 1, default_cap, plan).code == kInvalidArgument);

    if (check_shared_pieces())
        return 1;
    std::puts("ok");
    return 0;
}
