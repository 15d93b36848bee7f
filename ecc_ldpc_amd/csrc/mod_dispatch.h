// mod_dispatch.h -- the host side every launcher of the modulation files shares (the demappers demap*.hip, the frame source's modulated
// paths sim_mod*.hip): the run-time values that select a kernel instance (bits per symbol or per axis, the LLR output format, the LLR
// rule) turned into types for a generic lambda, the launch geometry, the launch-limit check and the launch-error check.  Host code only:
// no kernel lives here, and which instances exist is decided by the launcher that names its kernel inside the lambda.
#pragma once
#include "demap.h"
#include <algorithm>
#include <type_traits>

namespace ldpc {

template <int K> using Bits = std::integral_constant<int, K>;    // fn's argument k: decltype(k)::value is the template argument
template <typename T> struct Fmt { typedef T type; };            // fn's argument t: typename decltype(t)::type is the element type

// bits per symbol (a table object) or per axis (a product object), 1..6: fn(Bits<n>) -> its return code
template <class F>
static inline int dispatch_bits(const char *what, int n, F &&fn) {
    switch (n) {
        case 1: return fn(Bits<1>{});
        case 2: return fn(Bits<2>{});
        case 3: return fn(Bits<3>{});
        case 4: return fn(Bits<4>{});
        case 5: return fn(Bits<5>{});
        case 6: return fn(Bits<6>{});
        default: return set_error(LDPC_EINVAL, "%s: %d bits per symbol or axis", what, n);
    }
}

// the LLR output format (the entry points have checked it): fn(Fmt<float | __half | int8_t>)
template <class F>
static inline int dispatch_fmt(int fmt, F &&fn) {
    if (fmt == MOD_LLR_I8) return fn(Fmt<int8_t>{});
    if (fmt == MOD_LLR_F16) return fn(Fmt<__half>{});
    return fn(Fmt<float>{});
}

// the LLR rule of the modulation object: fn(Bits<DEMAP_MAXLOG | DEMAP_LOGMAP>)
template <class F>
static inline int dispatch_rule(int rule, F &&fn) {
    if (rule == DEMAP_LOGMAP) return fn(Bits<DEMAP_LOGMAP>{});
    return fn(Bits<DEMAP_MAXLOG>{});
}

// the instance of a generator kernel: fn(Bits<n>, Fmt<T>); of a demapper kernel: fn(Bits<rule>, Bits<n>, Fmt<T>)
template <class F>
static inline int dispatch_bits_fmt(const char *what, int n, int fmt, F &&fn) {
    return dispatch_bits(what, n, [&](auto k) { return dispatch_fmt(fmt, [&](auto t) { return fn(k, t); }); });
}
template <class F>
static inline int dispatch_rule_bits_fmt(const char *what, int rule, int n, int fmt, F &&fn) {
    return dispatch_rule(rule, [&](auto r) { return dispatch_bits_fmt(what, n, fmt, [&](auto k, auto t) { return fn(r, k, t); }); });
}

// ---- geometry.  A frame of n bits in symbols (or slots) of M bits; the frame source's kernels work a PAIR of them a lane
static inline int mod_symbols(int n, int M) { return (n + M - 1) / M; }
static inline int mod_pairs(int n_sym) { return (n_sym + 1) / 2; }
// lanes per frame of a kernel that writes through an interleaver: the items, then ceil(n_holes / K) lanes of K holes each
static inline int mod_lanes(int items, int n_holes, int K) { return items + (n_holes + K - 1) / K; }
// a pair's two samples (16 bytes) or two gains (8 bytes) go out in one store: every pair is whole and starts on that boundary
static inline int grant_pair_store(int n_sym, const void *p, int bytes) { return (n_sym % 2 == 0) && ((uintptr_t)p % bytes == 0); }
// a slot's M elements go out in vector stores of `bytes`: rows of whole slots in a buffer aligned to the piece
static inline bool grant_slot_store(int N, int M, const void *d_llr, size_t bytes) { return N % M == 0 && (uintptr_t)d_llr % bytes == 0; }
// grids of 256-lane blocks: one item a lane (demap_product.hip says which kernels have no grid-stride loop and why), or a grid-stride loop
static inline dim3 grid_lanes(size_t total) { return dim3((unsigned)((total + 255) / 256)); }
static inline dim3 grid_stride(size_t total) { return dim3((unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 20)); }

// the one-item-a-lane launchers refuse more items than a grid holds (demap.h kLaneMaxItems).  `of` names what was counted where that is
// a product of the caller's arguments ("batch * N"), null where it is lanes
static inline int check_items(const char *what, size_t items, const char *of = nullptr) {
    if (items <= kLaneMaxItems) return LDPC_OK;
    if (of) return set_error(LDPC_EINVAL, "%s: %s = %zu is more than one launch holds", what, of, items);
    return set_error(LDPC_EINVAL, "%s: %zu items are more than one launch holds", what, items);
}

// the end of every launcher: rc of the dispatch if that refused, else what the launch left behind
static inline int launched(const char *what, int rc = LDPC_OK) {
    if (rc != LDPC_OK) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "%s: %s", what, hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
