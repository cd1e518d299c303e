// lineclip_host_driver.cpp — the host-checkable part of csrc/gpk_lineclip.h (the crossing point around a local origin, the order of
// events with its exact tie rules, the run state machine) run on the CPU with an exact __int128 orientation (the fixture's coordinates
// are integers, at either placement).
//   lineclip_host_driver IN OUT
// IN is a sequence of records, one per segment:
//   int32 mode, int32 kept0 (the piece next to p is kept), double p[2], q[2], o[2] (the local origin), int32 n_events, then per event
//   int32 kind (0: ring vertex a on the open segment, 1: proper crossing with ring edge ab), int32 type (+1 entry, -1 exit, 0 no
//   transition — exact, from the reference), double a[2], b[2]
// in ANY order: the driver finds the next event from the current one exactly as the device routine does (the minimum under
// lc::earlier of the events after the current one), bounded by the number of events.
// OUT receives per record int32 n, then n times { int32 begin_part, int32 event (-1: p or q, else the record's event number),
// double x, y }: the calls the run state machine made on its sink.  Built by tests/test_lineclip_host.py with the host compiler,
// once plain and once with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_lineclip.h"

using gpk::lc::Event;
using gpk::lc::P2;

namespace {

struct ExactOrient {
    int operator()(P2 a, P2 b, P2 c) const {
        const __int128 ax = (int64_t)a.x, ay = (int64_t)a.y, bx = (int64_t)b.x, by = (int64_t)b.y, cx = (int64_t)c.x, cy = (int64_t)c.y;
        const __int128 d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
        return d > 0 ? 1 : (d < 0 ? -1 : 0);
    }
};

struct Out {
    int32_t begin, event;
    double x, y;
};

struct Sink {
    std::vector<Out> calls;
    bool pending = false;
    int event = -1;
    void begin_part() { pending = true; }
    void coord(P2 v) {
        calls.push_back(Out{pending ? 1 : 0, event, v.x, v.y});
        pending = false;
    }
};

template <typename T>
bool rd(FILE* f, T& v) {
    return fread(&v, sizeof v, 1, f) == 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t mode;
    while (rd(in, mode)) {
        int32_t kept0, n;
        P2 p, q, o;
        if (!rd(in, kept0) || !rd(in, p) || !rd(in, q) || !rd(in, o) || !rd(in, n) || n < 0) return 3;
        std::vector<Event> ev((size_t)n);
        std::vector<int32_t> type((size_t)n);
        for (int32_t k = 0; k < n; ++k) {
            int32_t kind;
            if (!rd(in, kind) || !rd(in, type[(size_t)k]) || !rd(in, ev[(size_t)k].a) || !rd(in, ev[(size_t)k].b)) return 3;
            ev[(size_t)k].kind = kind;
            ev[(size_t)k].id = 2 * k + kind;
            ev[(size_t)k].t = kind == 1 ? gpk::lc::crossing_t(p, q, ev[(size_t)k].a, ev[(size_t)k].b, o) : 0.0;
        }
        Sink sink;
        gpk::lc::Run run = gpk::lc::run_start();
        gpk::lc::run_segment_begin(run, kept0 != 0, p, sink);
        const Event none{-1, 0x7fffffff, p, p, 0.0};
        Event cur = none;
        for (int32_t it = 0; it < n; ++it) {
            Event best = none;
            for (const Event& e : ev)
                if (gpk::lc::event_before(cur, e, p, q, ExactOrient{})) best = gpk::lc::earlier(best, e, p, q, ExactOrient{});
            if (best.kind < 0) break;
            cur = best;
            const int32_t k = cur.id >> 1;
            sink.event = k;
            if (type[(size_t)k]) gpk::lc::run_transition(run, type[(size_t)k], cur.kind == 0 ? cur.a : gpk::lc::point_at(p, q, cur.t), sink);
        }
        sink.event = -1;
        gpk::lc::run_segment_end(run, q, sink);
        const int32_t m = (int32_t)sink.calls.size();
        fwrite(&m, sizeof m, 1, out);
        if (m) fwrite(sink.calls.data(), sizeof(Out), (size_t)m, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
