// aesgcm_dispatch.h -- from a launch's run-time arguments (rounds, mode or decrypt, lanes per packet, form) to the template arguments of the kernel instance that runs
// it, for every launcher of the library.  Two primitives over a compile-time list of ints, klist<V...>:
//     pick(klist, v, f)   f(kconst<V>{}) for the first V equal to v, for the LAST V if none is: the fall-through rule of every launcher ("nr anything else -> 14")
//     each(klist, f)      f(kconst<V>{}) for every V in order; f returns an error code (0 = success): the first error ends the walk and is returned
// and their products over a kset<klist...> (set_pick, set_each).  An instance set is written once, as a kset; its launcher picks from it with a generic lambda that
// names the kernel, and the attribute setter walks the same set:
//     batch3_dispatch(nr, dec, lg, [&](auto NR, auto D, auto LG) { hipLaunchKernelGGL((k<NR(), D(), LG()>), ..., dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), ...); });
//     batch3_each([](auto NR, auto D, auto LG) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k<NR(), D(), LG()>), ...); });
// No HIP header and no kernel's name in here, and the mode constants come in as template arguments: a host compiler alone builds against it
// (tests/test_dispatch_cpu.py checks the rules below for every input, and the size of every set).
#pragma once
#include <type_traits>

template <int V> using kconst = std::integral_constant<int, V>;
template <int... Vs> struct klist {};
template <class... Lists> struct kset {};

template <int V, int... Rest, class F> auto pick(klist<V, Rest...>, int v, F &&f) {
    if constexpr (sizeof...(Rest) == 0) return f(kconst<V>{});
    else {
        if (v == V) return f(kconst<V>{});
        return pick(klist<Rest...>{}, v, f);
    }
}
template <int V, int... Rest, class F> auto each(klist<V, Rest...>, F &&f) {
    auto e = f(kconst<V>{});
    if constexpr (sizeof...(Rest) != 0) { if (!e) return each(klist<Rest...>{}, f); }
    return e;
}
// the same over a product of lists: f(kconst...) with one constant of each list, picked by the values in the lists' order (set_pick) or for all of them (set_each: the first list slowest)
template <class F> auto set_pick(kset<>, F &&f) { return f(); }
template <class L, class... Ls, class F, class... Is> auto set_pick(kset<L, Ls...>, F &&f, int v, Is... vs) {
    return pick(L{}, v, [&](auto X) { return set_pick(kset<Ls...>{}, [&](auto... Ys) { return f(X, Ys...); }, vs...); });
}
template <class F> auto set_each(kset<>, F &&f) { return f(); }
template <class L, class... Ls, class F> auto set_each(kset<L, Ls...>, F &&f) {
    return each(L{}, [&](auto X) { return set_each(kset<Ls...>{}, [&](auto... Ys) { return f(X, Ys...); }); });
}
// sets one after the other, with each's rule for errors
template <class S, class... Ss, class F> auto sets_each(F &&f, S, Ss... more) {
    auto e = set_each(S{}, f);
    if constexpr (sizeof...(Ss) != 0) { if (!e) return sets_each(f, more...); }
    return e;
}

using nr_list = klist<10, 12, 14>;                     // nr 10 -> 10, 12 -> 12, anything else -> 14
using dec_list = klist<0, 1>;                          // dec 0 -> 0, anything else -> 1

// the kernels with NR alone (k_kt_setup, k_kt_quic_hp, the probe of k_batch3)
template <class F> auto nr_dispatch(int nr, F &&f) { return pick(nr_list{}, nr, f); }
template <class F> auto nr_each(F &&f) { return each(nr_list{}, f); }

// the kernels that run aesgcm_batch3_body.inc: f(NR, DEC, LG) for one / each of the 18 instances; lg 3 -> 3, 4 -> 4, anything else -> 6
using batch3_set = kset<nr_list, dec_list, klist<3, 4, 6>>;
template <class F> auto batch3_dispatch(int nr, int dec, int lg, F &&f) { return set_pick(batch3_set{}, f, nr, dec, lg); }
template <class F> auto batch3_each(F &&f) { return set_each(batch3_set{}, f); }

// ... with one more two-valued template argument, the family's variant (k_kt_wirex's extension, k_kt_tls's and k_kt_dtls's version, k_kt_srtp's kind): f(NR, DEC, LG, V),
// 36 instances.  v A -> A, anything else -> B: a launcher refuses an unknown variant before it dispatches
template <int A, int B> using batch3v_set = kset<nr_list, dec_list, klist<3, 4, 6>, klist<A, B>>;
template <int A, int B, class F> auto batch3v_dispatch(int nr, int dec, int lg, int v, F &&f) { return set_pick(batch3v_set<A, B>{}, f, nr, dec, lg, v); }
template <int A, int B, class F> auto batch3v_each(F &&f) { return set_each(batch3v_set<A, B>{}, f); }

// the two mask kernels, a lane per packet (k_kt_quic_hp, k_kt_dtls_sn): f(NR, DEC), 6 instances
using mask_set = kset<nr_list, dec_list>;
template <class F> auto mask_dispatch(int nr, int dec, F &&f) { return set_pick(mask_set{}, f, nr, dec); }
template <class F> auto mask_each(F &&f) { return set_each(mask_set{}, f); }

// k_main: f(NR, MODE); mode ENC / DEC / KS, anything else ECB.  12 instances
template <int ENC, int DEC, int KS, int ECB> using main_set = kset<nr_list, klist<ENC, DEC, KS, ECB>>;

// k_rows: f(NR, MODE) with MODE = dec ? DEC : ENC.  6 instances
template <int ENC, int DEC> using rows_set = kset<nr_list, klist<ENC, DEC>>;
template <int ENC, int DEC, class F> auto rows_dispatch(int nr, int dec, F &&f) { return set_pick(rows_set<ENC, DEC>{}, f, nr, dec ? DEC : ENC); }

// k_body and k_bodyh: f(NR, MODE, FORM).  The dealt chunks know DEC, PROBE and anything else as ENC (9 instances); the cyclic rows and their half shape DEC, anything
// else as ENC (6 each)
enum { BODY_DEALT = 0, BODY_CYC = 1, BODY_HALF = 2 };
template <int ENC, int DEC, int PROBE> struct body_sets {
    using dealt = kset<nr_list, klist<DEC, PROBE, ENC>, klist<BODY_DEALT>>;
    using cyc = kset<nr_list, klist<DEC, ENC>, klist<BODY_CYC>>;
    using half = kset<nr_list, klist<DEC, ENC>, klist<BODY_HALF>>;
};
template <int ENC, int DEC, int PROBE, class F> void body_dispatch(int nr, int mode, bool cyc, bool half, F &&f) {
    using S = body_sets<ENC, DEC, PROBE>;
    if (half) set_pick(typename S::half{}, f, nr, mode, BODY_HALF);
    else if (cyc) set_pick(typename S::cyc{}, f, nr, mode, BODY_CYC);
    else set_pick(typename S::dealt{}, f, nr, mode, BODY_DEALT);
}
template <int ENC, int DEC, int PROBE, class F> auto body_each(F &&f) {
    using S = body_sets<ENC, DEC, PROBE>;
    return sets_each(f, typename S::dealt{}, typename S::cyc{}, typename S::half{});
}

// The packet kernels under the context's key: f(NR, DEC, ILP or LG, SCATTERED).  DEC 2 is the probe, which exists for the shapes below and not for scattered messages
// (a dec of 2 lands on 1 there).  *_dispatch returns false, and calls nothing, for the inputs that have no instance.
// k_pktl (12 + 3 probes) and k_pktls (6; no ILP form: ilp is ignored)
using pktl_plain = kset<nr_list, dec_list, klist<0, 1>, klist<0>>;
using pktl_probe = kset<nr_list, klist<2>, klist<0>, klist<0>>;
using pktl_scattered = kset<nr_list, dec_list, klist<0>, klist<1>>;
template <class F> bool pktl_dispatch(int nr, int dec, bool ilp, bool scattered, F &&f) {
    if (scattered) set_pick(pktl_scattered{}, f, nr, dec, 0, 1);
    else if (dec == 2) { if (ilp) return false; set_pick(pktl_probe{}, f, nr, 2, 0, 0); }
    else set_pick(pktl_plain{}, f, nr, dec, ilp ? 1 : 0, 0);
    return true;
}
template <class F> auto pktl_each(F &&f) { return sets_each(f, pktl_plain{}, pktl_probe{}, pktl_scattered{}); }
// k_pktg (24: lg 2 / 3 / 4, anything else -> 6; + 9 probes) and k_pktgs (18).  The probes and the scattered form exist for lane groups of 4, 8 and 16 only
using pktg_plain = kset<nr_list, dec_list, klist<2, 3, 4, 6>, klist<0>>;
using pktg_probe = kset<nr_list, klist<2>, klist<2, 3, 4>, klist<0>>;
using pktg_scattered = kset<nr_list, dec_list, klist<2, 3, 4>, klist<1>>;
template <class F> bool pktg_dispatch(int nr, int dec, int lg, bool scattered, F &&f) {
    const bool small = lg == 2 || lg == 3 || lg == 4;
    if (scattered) { if (!small) return false; set_pick(pktg_scattered{}, f, nr, dec, lg, 1); }
    else if (dec == 2) { if (!small) return false; set_pick(pktg_probe{}, f, nr, 2, lg, 0); }
    else set_pick(pktg_plain{}, f, nr, dec, lg, 0);
    return true;
}
template <class F> auto pktg_each(F &&f) { return sets_each(f, pktg_plain{}, pktg_probe{}, pktg_scattered{}); }
