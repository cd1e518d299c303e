// gpk_scratch.h — the one way scratch is sized ("Scratch"): an entry point RECORDS its carves, commit() begins the arena with
// their sum + SCRATCH_TAIL and assigns every pointer in recorded order.  The slots must outlive commit(): locals of the entry point, or
// members of a struct it holds.  ScratchPlan is the arithmetic alone — no HIP call, no heap — so a host program can run it over a
// malloc'ed block (tests/scratch_host_driver.cpp, which defines GPK_SCRATCH_PLAN_ONLY).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/geopolars_hip.h"
#ifndef GPK_SCRATCH_PLAN_ONLY
#include "gpk_common.h"
#endif

namespace gpk {

constexpr size_t SCRATCH_TAIL = 1024;  // slack past the last carve (kernels that round a trailing vector access up)
constexpr int SCRATCH_SLOTS = 40;      // the polygon clip records the most, about 27

class ScratchPlan {
  public:
    static size_t aligned(size_t bytes) { return ((bytes ? bytes : 8) + 255) & ~size_t(255); }  // a carve of zero bytes still gets 8
    template <typename T>
    void add(T*& slot, size_t count) { record((void**)&slot, sizeof(T) * count, nullptr, false); }
    template <typename T>
    void add_bytes(T*& slot, size_t bytes) { record((void**)&slot, bytes, nullptr, false); }  // (T may be void)
    template <typename... T>
    void add_n(size_t count, T*&... slots) { (add(slots, count), ...); }  // several buffers of one length, in this order
    template <typename T>
    void add_if(bool cond, T*& slot, size_t count) {
        if (cond) add(slot, count); else slot = nullptr;
    }
    // an output of the caller's: used in place on the device, a carve (remembered for copy_back) on the host, nullptr when there is none
    template <typename T>
    void stage(T*& dev_slot, T* user_ptr, int32_t space, size_t count) {
        if (!user_ptr || space == GPK_MEM_DEVICE) dev_slot = user_ptr; else record((void**)&dev_slot, sizeof(T) * count, user_ptr, false);
    }
    // ... that the kernels write whether it was asked for or not: a plain carve when the caller passed none
    template <typename T>
    void stage_or_add(T*& dev_slot, T* user_ptr, int32_t space, size_t count) {
        if (user_ptr) stage(dev_slot, user_ptr, space, count); else add(dev_slot, count);
    }
    // an input of the caller's (a row list): the same as stage, remembered for upload
    template <typename T>
    void stage_in(const T*& dev_slot, const T* user_ptr, int32_t space, size_t count) {
        if (!user_ptr || space == GPK_MEM_DEVICE) dev_slot = user_ptr; else record((void**)&dev_slot, sizeof(T) * count, user_ptr, true);
    }
    bool ok() const { return !overflow_; }  // false: more than SCRATCH_SLOTS carves were asked for
    size_t total() const { return sum_ + SCRATCH_TAIL; }
    // every slot in recorded order; base is 256-aligned and holds total() bytes
    void assign(char* base) const {
        for (int i = 0; i < n_; ++i) *c_[i].slot = base + c_[i].offset;
    }

  protected:
    struct Carve {
        void** slot;
        size_t bytes, offset;  // bytes: as asked for (what a staged buffer's copy moves)
        const void* user;      // the caller's host buffer of a staged output or input, nullptr for a plain carve
        bool input;
    };
    Carve c_[SCRATCH_SLOTS];
    int n_ = 0;
    size_t sum_ = 0;
    bool overflow_ = false;
    void record(void** slot, size_t bytes, const void* user, bool input) {
        if (n_ == SCRATCH_SLOTS) {
            overflow_ = true;
            return;
        }
        c_[n_++] = Carve{slot, bytes, sum_, user, input};
        sum_ += aligned(bytes);
    }
};

#ifndef GPK_SCRATCH_PLAN_ONLY
class Scratch : public ScratchPlan {
  public:
    explicit Scratch(Workspace& ws) : ws_(ws) {}
    int32_t commit() {
        if (n_ == 0) return GPK_OK;  // nothing to carve: the arena is left as it is
        if (!ok()) return fail(GPK_ERR_INVALID_ARGUMENT, "scratch plan holds more than %d carves", SCRATCH_SLOTS);
        GPK_TRY(ws_.begin(total()));
        assign((char*)ws_.take(total()));
        return GPK_OK;
    }
    // after commit(): the host inputs that stage_in gave a carve reach it, in recorded order
    int32_t upload(hipStream_t s) const {
        for (int i = 0; i < n_; ++i)
            if (c_[i].input) GPK_HIP(hipMemcpyAsync(*c_[i].slot, c_[i].user, c_[i].bytes, hipMemcpyHostToDevice, s));
        return GPK_OK;
    }
    // copy_out of every host-staged output, in recorded order
    int32_t copy_back(hipStream_t s) const {
        for (int i = 0; i < n_; ++i)
            if (c_[i].user && !c_[i].input) GPK_TRY(copy_out(const_cast<void*>(c_[i].user), GPK_MEM_HOST, *c_[i].slot, c_[i].bytes, s));
        return GPK_OK;
    }

  private:
    Workspace& ws_;
};

// The one other protocol, for a build whose temporaries are sized by read-backs as it goes (the index build, the WKB decode): it reserves
// an ESTIMATE and carves while that lasts.  try_carve gives nullptr once the estimate is spent (or could not be had): the caller checks,
// and falls back to cached_malloc.
class ScratchEstimate {
  public:
    static void reserve(Workspace& ws, size_t estimate) { (void)ws.begin(estimate); }
    static void* try_carve(Workspace& ws, size_t bytes) { return ws.take(bytes); }
};
#endif

}  // namespace gpk
