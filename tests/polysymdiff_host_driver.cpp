// polysymdiff_host_driver.cpp — the host-checkable part of csrc/gpk_polysymdiff.h (the table of the symmetric difference as a rule
// type with the direction of a piece by its class) run on the CPU over the machinery of csrc/gpk_polyclip.h it uses: the side of a
// shared edge, the one value of a crossing, the arc state machine under a rule with directions by class (pc::turn_*: an arc end at
// every change of direction, the key of a backwards arc, the second lap when the first piece is kept backwards), the junction order
// at input coordinates and at computed crossings (pc::stitch<true>) and the stitcher with the innermost-shell nesting — the walk of
// tests/polyunion_host_driver.cpp with the branches pc::walk_ring_group takes under such a rule.  Orientation signs of lattice
// coordinates are exact (__int128; the fixture's coordinates are integers at either placement); a sign that involves a computed
// crossing is taken in extended precision — above the gap no such sign is near zero.
//   polysymdiff_host_driver IN OUT [ARCS]
// IN and OUT: the records of tests/polyunion_host_driver.cpp (tests/polysymdiff_ref.driver_records writes them, the touch points
// and classes being the exact ones of the reference, handed over in ANY order).  ARCS, when given, receives one int32 per pair: the
// number of arcs the two walks handed to the sink (-1 for a null pair) — what decides between the LDS slice and the global scratch
// of the device's stitch.
// Built by tests/test_polysymdiff_host.py with the host compiler, once plain and once with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_polysymdiff.h"

using gpk::lc::Event;
using gpk::lc::P2;
namespace pc = gpk::pc;
using Rule = gpk::ps::SymdiffRule;
static_assert(Rule::DIRECTION_BY_CLASS, "this driver walks the way of a rule with directions by class");

namespace {

struct Orient {
    int operator()(P2 a, P2 b, P2 c) const {
        const double v[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
        bool lattice = true;
        for (double x : v) lattice = lattice && x == std::floor(x) && std::fabs(x) < 9.0e15;
        if (lattice) {
            const __int128 ax = (int64_t)a.x, ay = (int64_t)a.y, bx = (int64_t)b.x, by = (int64_t)b.y, cx = (int64_t)c.x, cy = (int64_t)c.y;
            const __int128 d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
            return d > 0 ? 1 : (d < 0 ? -1 : 0);
        }
        const long double d = ((long double)b.x - a.x) * ((long double)c.y - a.y) - ((long double)b.y - a.y) * ((long double)c.x - a.x);
        return d > 0 ? 1 : (d < 0 ? -1 : 0);
    }
};

struct Piece {
    int32_t cls;
    P2 a, b;
    int32_t ccw, hole;
};

struct Ev {
    int32_t kind;
    P2 a, b;  // kind 0: a = b = the vertex
    Piece before, after;
    int32_t edge, ccw, hole, own;
    P2 own_v;
};

struct Sink {
    std::vector<pc::Arc> arcs;
    std::vector<P2> xy;
    pc::Arc cur{};
    void begin_arc(pc::End s, P2 s_nb, int key) {
        cur = pc::Arc{};
        cur.s = s;
        cur.s_nb = s_nb;
        cur.key = key;
        cur.c0 = (int)xy.size();
    }
    void coord(P2 v) { xy.push_back(v); }
    void end_arc(pc::End e, P2 e_nb, int flags) {
        cur.e = e;
        cur.e_nb = e_nb;
        cur.len = (int)xy.size() - cur.c0;
        cur.flags = flags;
        if (flags & pc::ARC_BACKWARDS) {  // the ends and the directions of the emitted arc
            std::swap(cur.s, cur.e);
            std::swap(cur.s_nb, cur.e_nb);
        }
        arcs.push_back(cur);
    }
    void rekey(int key) { cur.key = key; }
};

FILE* in;
template <typename T>
bool rd(T& v) {
    return fread(&v, sizeof v, 1, in) == 1;
}
bool rd_piece(Piece& p) { return rd(p.cls) && rd(p.a) && rd(p.b) && rd(p.ccw) && rd(p.hole); }

// the class of the piece t -> w
int cls_of(const Piece& p, P2 t, P2 w) {
    if (p.cls != 2) return p.cls == 1 ? pc::CLS_INTERIOR : pc::CLS_EXTERIOR;
    return pc::boundary_class(p.a, p.b, t, w, p.ccw, p.hole != 0);
}

struct Seg {
    int32_t seg, edge, p_on_boundary;
    P2 p, q, s0, s1;
    Piece first, last;
    std::vector<Ev> ev;
};

// walk_ring_group of the header, on the records of one ring
bool walk_ring(const std::vector<Seg>& segs, int c0, int walk, int mode, P2 o, Sink& out) {
    if (segs.empty()) return true;
    pc::Run run = pc::run_start();
    const P2 v0 = segs[0].p;
    int last_cls = 0, first_cls0 = 0;
    for (int lap = 0; lap < 2; ++lap) {
        if (lap == 1) {
            if (!run.head) {
                pc::turn_close_at_start(run, v0, segs[0].seg, walk, out);
                return true;
            }
            if (!run.any_break) {
                out.begin_arc(pc::end_at_coord(v0), segs[0].q, (walk == pc::WALK_B ? pc::KEY_WALK_B : 0) | (2 * c0));
                out.coord(v0);
                for (const Seg& s : segs) out.coord(s.q);
                int whole = segs[0].p_on_boundary && pc::is_cut_by<Rule>(last_cls, first_cls0, walk, mode) ? 0 : pc::ARC_WHOLE;
                if (Rule::backwards(first_cls0, walk, mode)) whole |= pc::ARC_BACKWARDS;
                out.end_arc(pc::end_at_coord(v0), run.prev_p, whole);
                return true;
            }
        }
        for (size_t k = 0; k < segs.size(); ++k) {
            const Seg& s = segs[k];
            const int first = cls_of(s.first, s.p, s.q);
            const bool had = run.started;
            if (!had) first_cls0 = first;
            pc::turn_segment_begin<Rule>(run, first, had && s.p_on_boundary && pc::is_cut_by<Rule>(last_cls, first, walk, mode), s.p, s.q, s.seg, walk, mode, out);
            if (lap == 1 && !run.open) return true;
            if (lap == 1) run.stop = true;
            const int n = (int)s.ev.size();
            std::vector<Event> ev((size_t)n);
            for (int i = 0; i < n; ++i) {
                ev[(size_t)i] = Event{s.ev[(size_t)i].kind, 2 * i + s.ev[(size_t)i].kind, s.ev[(size_t)i].a, s.ev[(size_t)i].b,
                                      s.ev[(size_t)i].kind == 1 ? gpk::lc::crossing_t(s.p, s.q, s.ev[(size_t)i].a, s.ev[(size_t)i].b, o) : 0.0};
            }
            const Event none{-1, 0x7fffffff, s.p, s.p, 0.0};
            Event cur = none;
            for (int it = 0; it < n; ++it) {
                Event best = none;
                for (const Event& e : ev)
                    if (gpk::lc::event_before(cur, e, s.p, s.q, Orient{})) best = gpk::lc::earlier(best, e, s.p, s.q, Orient{});
                if (best.kind < 0) break;
                cur = best;
                const Ev& e = s.ev[(size_t)(cur.id >> 1)];
                if (e.kind == 0) {
                    const int after = cls_of(e.after, e.a, s.q), before = pc::looking_back(cls_of(e.before, e.a, s.p));
                    pc::turn_at_vertex<Rule>(run, before, after, pc::end_at_coord(e.a), s.p, s.q, s.seg, walk, mode, out);
                } else {
                    const int ea = walk == pc::WALK_A ? s.edge : e.edge, eb = walk == pc::WALK_A ? e.edge : s.edge;
                    const bool a_left = walk == pc::WALK_A ? (s.p.x == s.s0.x && s.p.y == s.s0.y) : (e.ccw > 0) != (e.hole != 0);
                    const P2 x = walk == pc::WALK_A ? pc::crossing_point(s.s0, s.s1, e.a, e.b, o, a_left, Orient{})
                                                    : pc::crossing_point(e.a, e.b, s.s0, s.s1, o, a_left, Orient{});
                    const pc::End id = e.own ? pc::end_at_coord(e.own_v) : pc::End{x.x, x.y, ea, eb};
                    pc::turn_at_crossing(run, pc::class_after_crossing(Orient{}(e.a, e.b, s.q), e.ccw, e.hole != 0), id, s.p, s.q, s.seg, walk, out);
                }
                if (lap == 1 && !run.open) return true;
            }
            pc::turn_segment_end(run, s.p, s.q, out);
            last_cls = cls_of(s.last, s.q, s.p);
        }
    }
    pc::turn_close_at_start(run, v0, segs[0].seg, walk, out);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 2;
    in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    FILE* arcs_out = argc == 4 ? fopen(argv[3], "wb") : nullptr;
    if (!in || !out || (argc == 4 && !arcs_out)) return 2;
    int32_t mode;
    while (rd(mode)) {
        if (mode < 0) {
            const int32_t head[4] = {pc::ST_NULL, 0, 0, 0};
            fwrite(head, sizeof head, 1, out);
            const int32_t none = -1;
            if (arcs_out) fwrite(&none, sizeof none, 1, arcs_out);
            continue;
        }
        P2 o;
        if (!rd(o)) return 3;
        Sink sink;
        for (int walk = 0; walk < 2; ++walk) {
            int32_t n_rings;
            if (!rd(n_rings) || n_rings < 0) return 3;
            for (int32_t r = 0; r < n_rings; ++r) {
                int32_t c0, n_segs;
                if (!rd(c0) || !rd(n_segs) || n_segs < 0) return 3;
                std::vector<Seg> segs((size_t)n_segs);
                for (Seg& s : segs) {
                    int32_t n_ev;
                    if (!rd(s.seg) || !rd(s.edge) || !rd(s.p) || !rd(s.q) || !rd(s.s0) || !rd(s.s1) || !rd(s.p_on_boundary) || !rd_piece(s.first) ||
                        !rd_piece(s.last) || !rd(n_ev) || n_ev < 0)
                        return 3;
                    s.ev.resize((size_t)n_ev);
                    for (Ev& e : s.ev) {
                        if (!rd(e.kind)) return 3;
                        if (e.kind == 0) {
                            if (!rd(e.a) || !rd_piece(e.before) || !rd_piece(e.after)) return 3;
                            e.b = e.a;
                            e.edge = e.ccw = e.hole = e.own = 0;
                            e.own_v = e.a;
                        } else {
                            if (!rd(e.a) || !rd(e.b) || !rd(e.edge) || !rd(e.ccw) || !rd(e.hole) || !rd(e.own) || !rd(e.own_v)) return 3;
                            e.before = e.after = Piece{};
                        }
                    }
                }
                walk_ring(segs, c0, walk, mode, o, sink);
            }
        }
        const int n = (int)sink.arcs.size();
        const int32_t n_arcs = n;
        if (arcs_out) fwrite(&n_arcs, sizeof n_arcs, 1, arcs_out);
        std::vector<int> next((size_t)n + 1), ring_first((size_t)n + 1), order((size_t)n + 1), info((size_t)n + 1);
        int parts = 0, rings = 0, coords = 0;
        const int st = pc::stitch<true>(sink.arcs.data(), n, sink.xy.data(), Orient{}, next.data(), ring_first.data(), order.data(), info.data(), parts, rings, coords,
                                 /*innermost=*/true);
        const int32_t head[4] = {st <= pc::ST_TOUCH && parts == 0 ? pc::ST_EMPTY : st, parts, rings, coords};
        fwrite(head, sizeof head, 1, out);
        std::vector<int32_t> per_part, per_ring;
        std::vector<P2> xy;
        for (int j = 0; j < rings; ++j) {
            const int first = order[(size_t)j] & ~pc::ORDER_SHELL;
            if (order[(size_t)j] & pc::ORDER_SHELL) per_part.push_back(0);
            if (per_part.empty()) return 5;
            ++per_part.back();
            const size_t before = xy.size();
            int a = first;
            for (int it = 0; it < n; ++it) {
                const pc::Arc& A = sink.arcs[(size_t)a];
                for (int i = 0; i + 1 < A.len; ++i) xy.push_back(pc::arc_coord(A, sink.xy.data(), i));
                a = next[(size_t)a];
                if (a == first) break;
            }
            xy.push_back(pc::arc_coord(sink.arcs[(size_t)first], sink.xy.data(), 0));
            per_ring.push_back((int32_t)(xy.size() - before));
        }
        if ((int)per_part.size() != parts || (int)xy.size() != coords) return 6;
        if (parts) fwrite(per_part.data(), sizeof(int32_t), per_part.size(), out);
        if (rings) fwrite(per_ring.data(), sizeof(int32_t), per_ring.size(), out);
        if (coords) fwrite(xy.data(), sizeof(P2), xy.size(), out);
    }
    fclose(in);
    if (arcs_out && fclose(arcs_out) != 0) return 4;
    return fclose(out) == 0 ? 0 : 4;
}
