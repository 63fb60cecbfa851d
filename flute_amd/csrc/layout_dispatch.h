// The one ladder from a layer's runtime (dtype, num_bits, TileP) to template arguments.  The packed format has five
// layouts - (4, 32), (4, 64), (2, 32), (2, 64), (3, 32): 3-bit weights pack with TileP 32 only - each in f16 and bf16.
#pragma once
#include <type_traits>

#include "common.h"
#include "../../include/flute_amd.h"

namespace flute_amd {

template <int V> using int_c = std::integral_constant<int, V>;

// Calls f(T{}, int_c<BITS>{}, int_c<TILEP>{}) - T = F16 for FLUTE_F16, BF16 otherwise (the callers have checked dtype) -
// for the layout (num_bits, tile_p) names and returns FLUTE_OK; any other pair is FLUTE_ERR_TEMPLATE_ID and f is not
// called.  f is instantiated for exactly these ten combinations, so what it launches is too; a further axis of a
// site (a mode, a group size) is a choice inside f.
template <typename F>
int dispatch_layout(int dtype, int num_bits, int tile_p, F&& f) {
    auto typed = [&](auto bits, auto tp) {
        if (dtype == FLUTE_F16) f(F16{}, bits, tp);
        else f(BF16{}, bits, tp);
        return (int)FLUTE_OK;
    };
    if (num_bits == 4 && tile_p == 32) return typed(int_c<4>{}, int_c<32>{});
    if (num_bits == 4 && tile_p == 64) return typed(int_c<4>{}, int_c<64>{});
    if (num_bits == 2 && tile_p == 32) return typed(int_c<2>{}, int_c<32>{});
    if (num_bits == 2 && tile_p == 64) return typed(int_c<2>{}, int_c<64>{});
    if (num_bits == 3 && tile_p == 32) return typed(int_c<3>{}, int_c<32>{});
    return FLUTE_ERR_TEMPLATE_ID;
}

}  // namespace flute_amd
