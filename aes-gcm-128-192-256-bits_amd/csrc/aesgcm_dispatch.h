// aesgcm_dispatch.h -- from a launch's run-time (nr, dec, lg) to the template arguments of the kernels that run aesgcm_batch3_body.inc (k_batch3, k_kt_batch, k_kt_wire,
// k_kt_wirex, k_kt_tls, k_kt_quic), once for all of them.  A launcher hands a generic lambda that names its kernel:
//     batch3_dispatch(nr, dec, lg, [&](auto NR, auto D, auto LG) { hipLaunchKernelGGL((k<NR(), D(), LG()>), ..., dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), ...); });
// and its attribute setter one that returns an error:
//     batch3_each([](auto NR, auto D, auto LG) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k<NR(), D(), LG()>), ...); });
// No HIP header and no kernel's name in here: a host compiler alone builds against it (tests/test_dispatch_cpu.py checks the rules below for every input).
#pragma once
#include <type_traits>

template <int V> using kconst = std::integral_constant<int, V>;

// nr 10 -> 10, 12 -> 12, anything else -> 14 (also for the kernels with NR alone: k_kt_setup, k_kt_quic_hp)
template <class F> auto nr_dispatch(int nr, F &&f) {
    if (nr == 10) return f(kconst<10>{});
    if (nr == 12) return f(kconst<12>{});
    return f(kconst<14>{});
}

// f(NR, DEC, LG) for exactly one of the 18 instances; returns what f returns.  nr as above; dec 0 -> 0, anything else -> 1; lg 3 -> 3, 4 -> 4, anything else -> 6
template <class F> auto batch3_dispatch(int nr, int dec, int lg, F &&f) {
    return nr_dispatch(nr, [&](auto NR) {
        const auto with_lg = [&](auto D) {
            if (lg == 3) return f(NR, D, kconst<3>{});
            if (lg == 4) return f(NR, D, kconst<4>{});
            return f(NR, D, kconst<6>{});
        };
        if (dec) return with_lg(kconst<1>{});
        return with_lg(kconst<0>{});
    });
}

// f(NR) for 10, 12 and 14; f returns an error code (0 = success): the first error ends the walk and is returned
template <class F> auto nr_each(F &&f) {
    decltype(f(kconst<10>{})) e{};
    (void)((e = f(kconst<10>{})) || (e = f(kconst<12>{})) || (e = f(kconst<14>{})));
    return e;
}

// f(NR, DEC, LG) for each of the 18 instances, once, with nr_each's rule for errors
template <class F> auto batch3_each(F &&f) {
    return nr_each([&](auto NR) {
        decltype(f(NR, kconst<0>{}, kconst<3>{})) e{};
        const auto lgs = [&](auto D) { return (e = f(NR, D, kconst<3>{})) || (e = f(NR, D, kconst<4>{})) || (e = f(NR, D, kconst<6>{})); };
        (void)(lgs(kconst<0>{}) || lgs(kconst<1>{}));
        return e;
    });
}
