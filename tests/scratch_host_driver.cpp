// scratch_host_driver.cpp — the arithmetic of the scratch planner (csrc/gpk_scratch.h: record carves, sum them, assign the slots from a
// base pointer) run on the CPU over a malloc'ed block that stands in for the arena.  The block holds exactly total() - SCRATCH_TAIL
// bytes and every carve is filled to its last byte, so a sanitizer sees a carve that overlaps its neighbour or runs past the sum.
// A stand-alone program: tests/test_scratch_host.py builds it plain and with -fsanitize=address,undefined.  Prints "ok <checks>" and
// exits 0, or names the first check that failed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define GPK_SCRATCH_PLAN_ONLY
#include "gpk_scratch.h"

using gpk::SCRATCH_SLOTS;
using gpk::SCRATCH_TAIL;

// the planner, with its record readable
struct ScratchPlan : gpk::ScratchPlan {
    int count() const { return n_; }
    size_t offset(int i) const { return c_[i].offset; }
    size_t bytes(int i) const { return c_[i].bytes; }             // as asked for (the size of a staged buffer's copy)
    const void* staged_for(int i) const { return c_[i].user; }   // the caller's host buffer, nullptr for a plain carve
    bool is_input(int i) const { return c_[i].input; }            // uploaded after commit(), never copied back
};
static_assert(SCRATCH_TAIL == 1024, "the tail is the largest slack a hand-kept sum carried");
static_assert(SCRATCH_SLOTS == 40, "the polygon clip records about 27 carves");

static int n_checks = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        ++n_checks;                                                           \
        if (!(cond)) {                                                        \
            fprintf(stderr, "scratch_host_driver:%d: %s\n", __LINE__, #cond); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

// a 256-aligned block of exactly `bytes` bytes (what Workspace hands to the planner, without the tail)
struct Arena {
    char* base;
    size_t bytes;
    explicit Arena(size_t n) : base((char*)aligned_alloc(256, n ? n : 256)), bytes(n) {
        if (!base) exit(2);
    }
    ~Arena() { free(base); }
    bool holds(const void* p, size_t n) const { return (const char*)p >= base && (const char*)p + n <= base + bytes; }
};

// the carves of a call with every kind of record in it; `host`: the caller's buffers are on the host
struct Call {
    double* stats;
    int32_t *big, *none, *empty;
    void* raw;
    double* out_dev;
    uint8_t* valid_dev;
    int32_t* absent_dev;
    const uint32_t* rows_dev;
    double out_user[5];
    uint8_t valid_user[5];
    uint32_t rows_user[5];
    void plan(ScratchPlan& sc, bool host, bool with_none) {
        const int32_t space = host ? GPK_MEM_HOST : GPK_MEM_DEVICE;
        sc.add(stats, 37);                                 // 296 bytes: two units
        sc.add(big, 1000);                                 // 4000 bytes: no multiple of 256
        sc.add_if(with_none, none, 3);                     //
        sc.add(empty, 0);                                  // zero bytes still gets 8
        sc.add_bytes(raw, 257);                            //
        sc.stage(out_dev, out_user, space, 5);             //
        sc.stage(valid_dev, valid_user, space, 5);         //
        sc.stage(absent_dev, (int32_t*)nullptr, space, 5); // an output the caller did not ask for
        sc.stage_in(rows_dev, (const uint32_t*)rows_user, space, 5);
    }
};

static void fill(void* p, size_t n, int tag) { memset(p, tag, n ? n : 8); }

static void check_layout(bool host) {
    ScratchPlan sc;
    Call c;
    c.plan(sc, host, false);
    CHECK(sc.ok());
    CHECK(c.none == nullptr);  // a false add_if: nullptr at once, and nothing recorded
    CHECK(sc.count() == (host ? 7 : 4));

    // total == the aligned sizes + the tail, from the record and from the sizes written out by hand
    size_t sum = 0;
    for (int i = 0; i < sc.count(); ++i) {
        CHECK(sc.offset(i) == sum);
        sum += ScratchPlan::aligned(sc.bytes(i));
    }
    CHECK(sc.total() == sum + SCRATCH_TAIL);
    const size_t by_hand = 512 + 4096 + 256 + 512 + (host ? 256 + 256 + 256 : 0);
    CHECK(sum == by_hand);
    CHECK(ScratchPlan::aligned(0) == 256 && ScratchPlan::aligned(1) == 256 && ScratchPlan::aligned(256) == 256 && ScratchPlan::aligned(257) == 512);

    Arena a(sc.total() - SCRATCH_TAIL);
    sc.assign(a.base);
    void* slots[7] = {c.stats, c.big, c.empty, c.raw, c.out_dev, c.valid_dev, (void*)c.rows_dev};
    const size_t sizes[7] = {37 * 8, 4000, 0, 257, 40, 5, 20};
    const int n = sc.count();
    for (int i = 0; i < n; ++i) {
        CHECK(slots[i] != nullptr);
        CHECK(((uintptr_t)slots[i] & 255) == 0);
        CHECK((char*)slots[i] == a.base + sc.offset(i));                   // recorded order
        CHECK(a.holds(slots[i], sizes[i] ? sizes[i] : 8));                 // inside [base, base + total - SCRATCH_TAIL)
        if (i > 0) CHECK((char*)slots[i] >= (char*)slots[i - 1] + (sizes[i - 1] ? sizes[i - 1] : 8));  // no overlap
        CHECK(sc.bytes(i) == sizes[i]);
    }
    for (int i = 0; i < n; ++i) fill(slots[i], sizes[i], 0x40 + i);  // to the last byte: the sanitizer's part
    for (int i = 0; i < n; ++i) {                                       // ... and nobody wrote into a neighbour
        const unsigned char* p = (const unsigned char*)slots[i];
        const size_t m = sizes[i] ? sizes[i] : 8;
        CHECK(p[0] == 0x40 + i && p[m - 1] == 0x40 + i);
    }

    // stage: host -> a carve and a recorded copy of the right size; device -> the user's pointer and no copy; absent -> null
    CHECK(c.absent_dev == nullptr);
    if (host) {
        CHECK(c.out_dev != c.out_user && c.valid_dev != c.valid_user && c.rows_dev != c.rows_user);
        CHECK(sc.staged_for(4) == c.out_user && sc.bytes(4) == sizeof c.out_user);
        CHECK(sc.staged_for(5) == c.valid_user && sc.bytes(5) == sizeof c.valid_user);
        CHECK(sc.staged_for(6) == c.rows_user && sc.bytes(6) == sizeof c.rows_user);
        for (int i = 0; i < 7; ++i) CHECK(sc.is_input(i) == (i == 6));  // the outputs are copied back, the input is uploaded
        for (int i = 0; i < 4; ++i) CHECK(sc.staged_for(i) == nullptr);
    } else {
        CHECK(c.out_dev == c.out_user && c.valid_dev == c.valid_user && c.rows_dev == c.rows_user);
        for (int i = 0; i < n; ++i) CHECK(sc.staged_for(i) == nullptr);
    }
}

// a true add_if is an add
static void check_add_if() {
    ScratchPlan with, without;
    Call a, b;
    a.plan(with, true, true);
    b.plan(without, true, false);
    CHECK(with.count() == without.count() + 1);
    CHECK(with.total() == without.total() + 256);
    Arena ar(with.total() - SCRATCH_TAIL);
    with.assign(ar.base);
    CHECK(a.none != nullptr && (char*)a.none == ar.base + 512 + 4096);
    fill(a.none, 12, 0x11);
}

// add_n: several buffers of one LENGTH, each sized by its own type, in the order given
static void check_add_n() {
    ScratchPlan sc;
    uint32_t *cand_r, *cand_l;
    uint8_t* hit;
    double* dist;
    sc.add_n(100, cand_r, cand_l, hit, dist);
    CHECK(sc.ok() && sc.count() == 4);
    CHECK(sc.bytes(0) == 400 && sc.bytes(1) == 400 && sc.bytes(2) == 100 && sc.bytes(3) == 800);
    CHECK(sc.offset(0) == 0 && sc.offset(1) == 512 && sc.offset(2) == 1024 && sc.offset(3) == 1280);
    CHECK(sc.total() == 1280 + 1024 + SCRATCH_TAIL);
    Arena a(sc.total() - SCRATCH_TAIL);
    sc.assign(a.base);
    CHECK((char*)cand_r == a.base && (char*)cand_l == a.base + 512 && (char*)hit == a.base + 1024 && (char*)dist == a.base + 1280);
    fill(cand_r, 400, 1), fill(cand_l, 400, 2), fill(hit, 100, 3), fill(dist, 800, 4);
    CHECK(((unsigned char*)cand_l)[399] == 2 && hit[0] == 3 && hit[99] == 3 && ((unsigned char*)dist)[0] == 4);
}

// stage_or_add: an output the kernels write whether the caller asked for it or not
static void check_stage_or_add() {
    int32_t user[6];
    for (int given = 0; given < 2; ++given)
        for (int host = 0; host < 2; ++host) {
            ScratchPlan sc;
            int32_t* dev = nullptr;
            sc.stage_or_add(dev, given ? user : (int32_t*)nullptr, host ? GPK_MEM_HOST : GPK_MEM_DEVICE, 6);
            if (given && !host) {  // the caller's device buffer, in place
                CHECK(dev == user && sc.count() == 0 && sc.total() == SCRATCH_TAIL);
                continue;
            }
            CHECK(sc.count() == 1 && sc.bytes(0) == sizeof user && sc.total() == 256 + SCRATCH_TAIL);
            CHECK(sc.staged_for(0) == (given ? user : nullptr) && !sc.is_input(0));  // copied back only when there is somewhere to
            Arena a(256);
            sc.assign(a.base);
            CHECK((char*)dev == a.base);
            fill(dev, sizeof user, 7);
        }
}

// one carve more than the capacity: a status, and nothing is written — to the slots or to the arena
static void check_overflow() {
    ScratchPlan sc;
    static int32_t* slots[SCRATCH_SLOTS + 1];
    int32_t* const poison = (int32_t*)(uintptr_t)0x5a5a00;
    for (int i = 0; i <= SCRATCH_SLOTS; ++i) slots[i] = poison;
    for (int i = 0; i < SCRATCH_SLOTS; ++i) sc.add(slots[i], 10);
    CHECK(sc.ok() && sc.count() == SCRATCH_SLOTS);
    const size_t total = sc.total();
    sc.add(slots[SCRATCH_SLOTS], 10);
    CHECK(!sc.ok());
    CHECK(sc.count() == SCRATCH_SLOTS && sc.total() == total);
    for (int i = 0; i <= SCRATCH_SLOTS; ++i) CHECK(slots[i] == poison);  // (commit() returns the status before it assigns)

    // exactly the capacity is fine, and fills
    ScratchPlan full;
    for (int i = 0; i < SCRATCH_SLOTS; ++i) full.add(slots[i], 10);
    CHECK(full.ok());
    Arena a(full.total() - SCRATCH_TAIL);
    full.assign(a.base);
    for (int i = 0; i < SCRATCH_SLOTS; ++i) {
        CHECK((char*)slots[i] == a.base + 256 * (size_t)i);
        fill(slots[i], 40, i);
    }
}

// the same carves recorded twice: the same offsets (what the join's tag relies on: its record lands at the same place)
static void check_repeat() {
    size_t offsets[2][8], totals[2];
    for (int round = 0; round < 2; ++round) {
        ScratchPlan sc;
        Call c;
        c.plan(sc, true, true);
        CHECK(sc.count() == 8);
        for (int i = 0; i < 8; ++i) offsets[round][i] = sc.offset(i);
        totals[round] = sc.total();
    }
    CHECK(totals[0] == totals[1]);
    for (int i = 0; i < 8; ++i) CHECK(offsets[0][i] == offsets[1][i]);
}

int main() {
    check_layout(true);
    check_layout(false);
    check_add_if();
    check_add_n();
    check_stage_or_add();
    check_overflow();
    check_repeat();
    printf("ok %d\n", n_checks);
    return 0;
}
