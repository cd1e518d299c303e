// gpk_polyunion.h — the area either of two polygonal rows covers: gpk_polygon_union (include/geopolars_hip.h; DESIGN.md section
// 4.3r).  a, b = POLYGON / MULTIPOLYGON rows.
//   GPK_PUNION_UNION  the closure of int(a) ∪ int(b) together with the shared boundary across which the two merge
// REGULARISED like gpk_polygon_clip: the area part only.
//
// The rule is that of gpk_polyclip.h — rule 1 (walks), rule 3 (arcs and their exact end identities), rule 4 (junctions: the leftmost
// turn, cuts at touch points), rule 5 (ring signs, ring starts, part order) and rule 6 (the contract) hold word for word — with another
// kept table and another choice of a hole's shell.
//
// Kept pieces.  The piece classes and the side of a shared edge are exactly pc::boundary_class's.
//     walk              UNION keeps
//     ∂a against b      EXTERIOR; BOUNDARY same side
//     ∂b against a      EXTERIOR only
// Shared boundary comes from a, never from b: equal polygons unite to a.  A shared edge with the interiors on opposite sides
// vanishes: neighbours that share an edge merge across it, and the input coordinates along the merged edge that are ends of kept
// pieces stay coordinates of the result, bit for bit, collinear or not.  Nothing is emitted backwards: every kept piece has the
// result on its left in its walk's direction.  At most one arc starts at any computed crossing — a proper crossing is left by the
// one of the two boundaries that goes on outside the other row — so the arc state machine and the stitcher of gpk_polyclip.h serve
// unchanged, and the junction rule is needed at input coordinates only, as there.  Consequences of rule 4, as there: rows that
// touch at a point unite to separate parts; rows that touch at two points around a gap unite to two parts and NO hole (each arc
// turns leftmost at the touch point, back onto its own row); a gap closed off by overlapping pieces is a hole made of arcs of both rows.
//
// The crossing value.  A crossing keeps its ONE value, pc::crossing_point: along a's edge, moved onto a's inner side.  No covered-by
// claim is made for a union; the contract is rule 6's: input coordinates bit for bit, crossings within 1e-9 d of both carrying
// edges, and the same gap condition 1e-6 |segment|, below which a row is within 1e-9 d or has status 4 and is null.
//
// Nesting.  Rule 5 of gpk_polyclip.h gives a hole to the first shell in key order that encloses it, which is right where no shell
// of a result lies inside a hole of another one.  A union has such shells: an annulus b inside the hole of an annulus a leaves two
// shells that both enclose b's hole, and a's comes first in key order.  Here a hole goes to the INNERMOST enclosing shell: the
// enclosing shell that every other enclosing shell encloses, both decided by pc::ring_encloses (pc::stitch with innermost = true;
// the clip modes leave the parameter off and their results do not move).  The shells that enclose a hole are nested in each other,
// so there is one.
//
// A null row: the conditions of gpk_polygon_clip.  A row without a coordinate on either side gives null — the pair-wise union does
// NOT treat an empty row as the neutral element (gpk_union_all_pairs, below, drops such rows before it pairs).
//
// Schedule: gpk_polyclip_run.h, shared with gpk_polygon_clip, instantiated with UnionRule: count, scan, fill, stitch (LDS slice or
// global scratch), scan, emit; G lanes per pair by lp::relation_group_size (4 and 16); every branch around a DPP reduction
// group-uniform.  Rows of many thousand coordinates run on the same lanes: correct and slow.
//
// What is new here — the kept table — is plain C++; tests/polyunion_host_driver.cpp runs it, with the arc machine and the stitcher
// of gpk_polyclip.h, on the CPU.
#pragma once

#include "gpk_polyclip.h"

namespace gpk {
namespace pu {

constexpr int MODE_UNION = 0;

// the kept table
GPK_LC_FN bool kept(int cls, int walk, int mode) {
    (void)mode;
    if (walk == pc::WALK_B) return cls == pc::CLS_EXTERIOR;
    return (cls & (pc::CLS_EXTERIOR | pc::CLS_BOUNDARY_SAME)) != 0;
}
GPK_LC_FN bool emitted_backwards(int, int) { return false; }

// the rule type the walks, pc::crossing_type_by and pc::is_cut_by take
struct UnionRule {
    static constexpr bool DIRECTION_BY_CLASS = false;
    static GPK_LC_FN bool kept(int cls, int walk, int mode) { return pu::kept(cls, walk, mode); }
    static GPK_LC_FN bool emitted_backwards(int walk, int mode) { return pu::emitted_backwards(walk, mode); }
};

// One round of a grouped union (gpk_union_all_pairs): `group` holds the sorted group ids of the current rows.  Row i is the
// (i - first row of its group)-th of its group; rows 2j and 2j + 1 of a group are united, an odd last row passes through.
// 0: row i opens a pair (with row i + 1), 1: it closes one, 2: it passes through.
GPK_LC_FN int union_all_role(const int32_t* group, int64_t n, int64_t i, int64_t first_of_group) {
    if (((i - first_of_group) & 1) != 0) return 1;
    return i + 1 < n && group[i + 1] == group[i] ? 0 : 2;
}

}  // namespace pu
}  // namespace gpk
