// dispatch.h -- which template instantiation serves a run-time value: each such decision of the launchers, once.
// No HIP in here (plain C++17), so that tests/host_hooks.cpp checks the choices on the CPU.  A functor receives its
// choice as std::integral_constant arguments, which convert to int in constant expressions: k_name<nch, me>.
#pragma once
#include <type_traits>
#include <utility>

template <int V> using int_c = std::integral_constant<int, V>;

// f(int_c<Vi>) for the Vi equal to v, and what it returns; `miss`, without calling f, when v is none of them
template <int... Vs, class R, class F>
inline R pick_int(int v, R miss, F&& f) {
  R r = miss;
  (void)((v == Vs ? (r = f(int_c<Vs>{}), true) : false) || ...);
  return r;
}

// The <NCH, ME> instantiation of the envelope kernels for nch channels of me envelope harmonics each (up to 8 and 8:
// the registers a lane holds them in come in these three sizes)
template <class F>
inline auto with_env_shape(int nch, int me, F&& f) {
  if(nch <= 4 && me <= 4) return f(int_c<4>{}, int_c<4>{});
  if(nch <= 4) return f(int_c<4>{}, int_c<8>{});
  return f(int_c<8>{}, int_c<8>{});
}

// Column tiles of a harmonic frame of nwin samples: row length L = 32 T - 2 samples (16 rows cover nwin), that is
// L / 2 + 1 = 16 T offsets from the row centre, in passes of NT <= 4 column tiles
struct SynthTiles { int T, NT, L; };
inline SynthTiles synth_tiles(int nwin) {
  int T = ((nwin + 15) / 16 + 2 + 31) / 32;
  int NT = T;
  if(T > 4) { T = (T + 3) / 4 * 4; NT = 4; }
  return {T, NT, 32 * T - 2};
}
// the <NTS> instantiation for SynthTiles::NT
template <class F>
inline auto with_tiles(int NT, F&& f) {
  switch(NT) {
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    case 3: return f(int_c<3>{});
    default: return f(int_c<4>{});
  }
}
