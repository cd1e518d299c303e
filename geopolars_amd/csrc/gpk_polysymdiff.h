// gpk_polysymdiff.h — the area exactly one of two polygonal rows covers: gpk_polygon_symdiff (include/geopolars_hip.h; DESIGN.md
// section 4.3w).  a, b = POLYGON / MULTIPOLYGON rows.
//   GPK_PSYMDIFF_SYMMETRIC_DIFFERENCE  the closure of (int(a) \ b) ∪ (int(b) \ a)
// REGULARISED like gpk_polygon_clip and gpk_polygon_union: the area part only.
//
// The rule is that of gpk_polyclip.h — rule 1 (walks), rule 3 (arcs and their exact end identities), rule 5 (ring signs, ring
// starts, part order) and rule 6 (the contract, without the covered-by claim) hold — with another kept table, a DIRECTION that goes
// by the class of a piece, junctions at computed crossings as well, and the union's choice of a hole's shell.
//
// Kept pieces.  The piece classes and the side of a shared edge are exactly pc::boundary_class's.
//     walk              EXTERIOR                INTERIOR                  BOUNDARY (same or opposite side)
//     ∂a against b      kept, emitted forwards  kept, emitted BACKWARDS   dropped
//     ∂b against a      kept, emitted forwards  kept, emitted BACKWARDS   dropped
// A piece of one boundary outside the other row bounds the part of its own row that is in the result: the result is on its left,
// as the row's interior is.  A piece INSIDE the other row has its own row's interior on its left, which there is NOT in the result,
// and the other row alone on its right, which is: the result is on its right and the piece is emitted backwards.  A shared edge
// with the interiors on the same side has both rows on one side and neither on the other: no side is in the result.  A shared edge
// with the interiors on opposite sides has exactly one row on either side: both sides are in the result, the edge vanishes and the
// two rows merge across it.  Consequences:
//   - equal polygons give an empty row: status ST_EMPTY, zero parts;
//   - neighbours that share an edge give their union;
//   - b strictly inside a gives a with b as a hole; a hole of b is then a shell inside that hole.
//
// Direction by class (SymdiffRule::DIRECTION_BY_CLASS; pc::turn_*).  Under the clip's and the union's tables a walk is emitted one
// way throughout.  Here a boundary that properly crosses the other row goes EXTERIOR -> INTERIOR, stays kept and TURNS ROUND: the arc
// ends there, with the identity of the crossing (ea, eb), and a new arc begins in the other direction, End::far and Arc::s_nb /
// e_nb taken from the segment's ends as at every other arc end.  An arc is stored in walk order; a backwards one is flagged
// ARC_BACKWARDS and read through pc::arc_coord, its ends and direction neighbours are those of the EMITTED direction; a ring kept
// whole inside the other row is ARC_WHOLE | ARC_BACKWARDS.
// Key convention: the key of an arc is that of its start in the emitted direction.  A backwards arc starts, as emitted, where the
// walk leaves it: its key is (walk << 30) | 2 * (the segment the walk is on at that moment) | (1 when that is inside the segment);
// an arc that ends at a coordinate of its ring has the number of the segment that begins there.  A forwards and a backwards arc
// of one walk that start at the same point share a key, and the backwards one comes first (it has the lower arc number).
//
// Junctions (rule 4, extended).  At a proper crossing two arcs END — the arc of the boundary that enters the other row and, backwards,
// the arc of that boundary inside it — and two START, along the two halves of the other boundary; all four carry the identity
// (ea, eb) and the ONE value pc::crossing_point gives.  The leftmost turn runs there too: an arc that arrives along the carrier
// e_nb -> far goes on along the half of the other carrier whose end lies to its LEFT, one exact orientation sign of four INPUT
// coordinates (pc::stitch<true>); the computed value is never read.  So a \ b and b \ a, which meet at the crossing as opposite
// wedges, touch there and stay separate rings, as parts that touch at an input coordinate do.  pc::ring_corners gives a corner at
// a crossing the carriers of the two arcs OF ITS RING that meet there, and pc::ring_sign turns on those: that a second ring
// passes through the same crossing, in the opposite wedge, does not enter.  pc::ring_encloses finds a crossing shared with the
// candidate shell ON it (both rings emit the same double) and goes on to the next coordinate.
//
// Nesting: a hole goes to the INNERMOST enclosing shell, as in gpk_polyunion.h (an annulus b in the hole of an annulus a).
//
// A null row: the conditions of gpk_polygon_clip.  A row without a coordinate on either side gives null, as in the union: an empty
// row is not treated as the neutral element.
//
// Schedule: gpk_polyclip_run.h instantiated with SymdiffRule.  A pair has up to about twice the union's arcs.
//
// What is new here — the table, the direction of a piece, with pc::turn_* and pc::stitch<true> of gpk_polyclip.h — is plain C++;
// tests/polysymdiff_host_driver.cpp runs it on the CPU.
#pragma once

#include "gpk_polyclip.h"

namespace gpk {
namespace ps {

constexpr int MODE_SYMMETRIC_DIFFERENCE = 0;

// the kept table: the same for both walks
GPK_LC_FN bool kept(int cls, int walk, int mode) {
    (void)walk;
    (void)mode;
    return (cls & (pc::CLS_INTERIOR | pc::CLS_EXTERIOR)) != 0;
}
// the direction of a kept piece
GPK_LC_FN bool backwards(int cls, int walk, int mode) {
    (void)walk;
    (void)mode;
    return cls == pc::CLS_INTERIOR;
}

// the rule type the walks take
struct SymdiffRule {
    static constexpr bool DIRECTION_BY_CLASS = true;
    static GPK_LC_FN bool kept(int cls, int walk, int mode) { return ps::kept(cls, walk, mode); }
    static GPK_LC_FN bool backwards(int cls, int walk, int mode) { return ps::backwards(cls, walk, mode); }
    static GPK_LC_FN bool emitted_backwards(int, int) { return false; }  // (no walk is backwards as a whole)
};

}  // namespace ps
}  // namespace gpk
