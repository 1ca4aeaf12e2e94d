// What vi_basis.hip, vi_eval.hip, vi_track.hip and vi_slant.hip share on the host beside the functions vi_solver.h declares: the
// dispatch of a model's order to the compiled kernel orders and the argument checks their entries repeat.
#pragma once
#include "vi_solver.h"

// The orders (MAXL, MAXK) the tiled kernels k_eval_sph_fast, k_track_sph_fast and k_slant_sph_fast are compiled at: X(L, K) for
// each.  The first two are the orders of the fp32-chain tolerance sweep (vi_model_set_eval_precision), the only ones compiled
// with float chains.
#define VI_FAST_ORDERS_F32(X) X(6, 4) X(2, 8)
#define VI_FAST_ORDERS(X) VI_FAST_ORDERS_F32(X) X(3, 4) X(4, 3) X(3, 2) X(12, 2) X(12, 8)

// *rc = f(integral_constant L, K) and true if the model's order is one of that list - of its fp32 part alone with F32_ONLY, so
// that a float instantiation exists for those two orders only -, else false: the caller goes on to the per-lane kernels.
template <bool F32_ONLY = false, class F>
bool at_fast_order(const vi_model* m, int* rc, F&& f)
{
    const int L = m->sph.maxl, K = m->sph.maxk;
#define VI_AT(LL, KK) \
    if (L == LL && K == KK) return *rc = f(std::integral_constant<int, LL>{}, std::integral_constant<int, KK>{}), true;
    if constexpr (F32_ONLY) {
        VI_FAST_ORDERS_F32(VI_AT)
    } else {
        VI_FAST_ORDERS(VI_AT)
    }
#undef VI_AT
    return false;
}

// The per-lane kernels (k_basis_sph, k_eval_sph, k_track_sph) are compiled at three caps (LCAP, KCAP): the default order, the
// C5 order, larger orders.  f(integral_constant LCAP, KCAP) at the first cap that holds the model's order.
template <class F>
int at_order_cap(const vi_model* m, const char* who, F&& f)
{
    const int L = m->sph.maxl, K = m->sph.maxk;
#define VI_CAP(LC, KC) \
    if (L <= LC && K <= KC) return f(std::integral_constant<int, LC>{}, std::integral_constant<int, KC>{});
    VI_CAP(6, 4) VI_CAP(12, 8) VI_CAP(24, 16)
#undef VI_CAP
    vi_set_error("%s: order MAXL=%d MAXK=%d beyond the compiled limits (24, 16)", who, L, K);
    return VI_ERR_UNSUPPORTED;
}

// The gradient kernels (k_grad_sph, k_track_grad_sph) are compiled at (MAXL, MAXK) up to (6, 4), (12, 8) or (2, 12):
// f(integral_constant LCAP, KCAP) at the first of those orders that holds the model's
template <class F>
int at_grad_cap(const vi_model* m, const char* who, F&& f)
{
    const int L = m->sph.maxl, K = m->sph.maxk;
#define VI_CAP(LC, KC) \
    if (L <= LC && K <= KC) return f(std::integral_constant<int, LC>{}, std::integral_constant<int, KC>{});
    VI_CAP(6, 4) VI_CAP(12, 8) VI_CAP(2, 12)
#undef VI_CAP
    vi_set_error("%s: order MAXL=%d MAXK=%d beyond the compiled limits (6, 4), (12, 8) and (2, 12)", who, L, K);
    return VI_ERR_UNSUPPORTED;
}

// The argument checks of the entries, once per kind of argument.  Macros: the message names the entry they stand in (__func__).
// VI_REQUIRE_RECORDS: R records whose rows (`what`: "coefficients", "covariances") are at d_rows.
#define VI_REQUIRE_HULL(F, d_hull_eq) VI_REQUIRE((F) == 0 || (d_hull_eq), "hull facet count given without facet equations")
#define VI_REQUIRE_FRAME(frame) \
    VI_REQUIRE((frame) == VI_FRAME_MODEL || (frame) == VI_FRAME_ENU, "frame must be VI_FRAME_MODEL or VI_FRAME_ENU")
#define VI_REQUIRE_RECORDS(R, d_rows, what)                                          \
    do {                                                                             \
        VI_REQUIRE((R) == 0 || (d_rows), "record count given without " what);        \
        VI_REQUIRE((R) <= 0x7fffffffLL, "more records than a 32-bit record index");  \
    } while (0)
#define VI_REQUIRE_RULE(n) VI_REQUIRE((n) >= 1, "a rule has at least one node")
#define VI_REQUIRE_RAYS(P) VI_REQUIRE((P) <= 0x7fffffffLL, "more rays than one launch takes")
