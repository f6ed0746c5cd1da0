// Stand-alone host program for ufr_igemm_tail_plan (csrc/igemm.hip), meant to be built with the host side under AddressSanitizer
// and UBSan (tests/test_igemm_tail_plan_host_cpu.py: hipcc -Xarch_host -fsanitize=address,undefined) and run WITHOUT a GPU: the
// plan is host arithmetic, no HIP call, no pointer dereferenced.  It sweeps (M, Npad, K tiles, resident workgroups), re-derives
// every field of a plan that is on from the rule in include/ufr_hip.h, and checks that every refused configuration is off.
// ufr_igemm_balanced is called only where it is refused before it asks for a device (a workspace that is too small).
#include <cstdio>
#include <cstring>

#include "../../include/ufr_hip.h"

static int failures = 0;
static long plans_on = 0, plans_off = 0;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      std::printf("FAIL ");         \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
      ++failures;                   \
    }                               \
  } while (0)

static ufr_igemm_desc make(long M, int Npad, int taps, int KC) {
  ufr_igemm_desc d;
  std::memset(&d, 0, sizeof d);
  d.B = 1; d.Hr = 1; d.Wr = (int)M;
  d.Hi = 1; d.Wi = (int)M; d.Ho = 1; d.Wo = (int)M;
  d.in_sy = d.in_sx = d.out_sy = d.out_sx = 1;
  d.KC = KC; d.Npad = Npad; d.N = Npad;
  d.nphase = 1; d.phase[0].ntaps = taps;
  d.splitk = 1; d.products = 6; d.variant = 6;
  return d;
}

static void check_plan(const ufr_igemm_desc& d, int R, const ufr_igemm_tail_plan_t& p) {
  const long M = (long)d.B * d.Hr * d.Wr;
  const int Mt = (int)((M + 255) / 256), Nt = d.Npad / 128, kt = d.phase[0].ntaps * d.KC;
  const long T = (long)Mt * Nt, q = T / R;
  CHECK(p.row_tiles == Mt && p.ktiles == kt, "M=%ld: row tiles %d, K tiles %d", M, p.row_tiles, p.ktiles);
  if (!p.on) {
    ++plans_off;
    bool want = d.Npad % 128 == 0 && d.nphase == 1 && d.variant == 6 && d.products == 6 && !d.tickets && !d.no_reduce && !d.tail &&
                d.splitk == 1 && q >= 1 && T % R != 0;
    if (want) {
      const long tiles = (long)(Mt - (int)(q * R / Nt)) * Nt;
      long S = R / tiles;
      if (S > kt / 8) S = kt / 8;
      if (S > 8) S = 8;
      want = S >= 2 && q * (kt + 6) + (kt + S - 1) / S + 6 + 10 <= ((T + R - 1) / R) * (kt + 6);
    }
    CHECK(!want, "M=%ld N=%d kt=%d R=%d: off where the rule says on", M, d.Npad, kt, R);
    CHECK(p.full_row_tiles == Mt && p.tail_row_tiles == 0 && p.ws_floats == 0 && p.slices == 0, "M=%ld N=%d kt=%d R=%d: an off plan has a tail", M,
          d.Npad, kt, R);
    return;
  }
  ++plans_on;
  CHECK(q >= 1 && T % R != 0, "M=%ld N=%d kt=%d R=%d: on without an under-filled last round", M, d.Npad, kt, R);
  CHECK(p.full_row_tiles + p.tail_row_tiles == Mt && p.full_row_tiles == (int)(q * R / Nt), "M=%ld R=%d: full %d + tail %d of %d", M, R,
        p.full_row_tiles, p.tail_row_tiles, Mt);
  CHECK(p.tail_row0 == p.full_row_tiles * 256 && (long)p.tail_row0 + p.tail_rows == M && p.tail_rows > 0, "M=%ld R=%d: tail rows [%d, +%d)", M, R,
        p.tail_row0, p.tail_rows);
  const long tiles = (long)p.tail_row_tiles * Nt;
  long S = R / tiles;
  if (S > kt / 8) S = kt / 8;
  if (S > 8) S = 8;
  CHECK(p.slices == S && S >= 2 && S * tiles <= R, "M=%ld N=%d kt=%d R=%d: %d slices, rule says %ld", M, d.Npad, kt, R, p.slices, S);
  CHECK(p.slice_ktiles == (kt + p.slices - 1) / p.slices && p.slice_ktiles >= 8 && (long)(p.slices - 1) * p.slice_ktiles < kt,
        "M=%ld kt=%d R=%d: slices of %d", M, kt, R, p.slice_ktiles);
  CHECK(p.workgroups == (long)p.full_row_tiles * Nt + tiles * p.slices, "M=%ld R=%d: %d workgroups", M, R, p.workgroups);
  CHECK(p.ws_floats == (long)p.slices * p.tail_rows * d.Npad, "M=%ld R=%d: workspace %ld", M, R, p.ws_floats);
  CHECK(p.steps_before == (int)((T + R - 1) / R) * (kt + 6) && p.steps_after == (int)q * (kt + 6) + p.slice_ktiles + 6 + 10 &&
            p.steps_after <= p.steps_before,
        "M=%ld kt=%d R=%d: steps %d -> %d", M, kt, R, p.steps_before, p.steps_after);
}

int main() {
  ufr_igemm_tail_plan_t p;
  // the sweep: row counts around tile and round boundaries, 1 .. 8 column tiles, short and long reductions, small and real chips
  const long Ms[] = {1, 255, 256, 257, 1920, 2400, 4096, 5000, 21504, 21505, 61440, 65536, 65537, 131072, 1000003};
  const int Ns[] = {128, 256, 384, 512, 1024};
  const int KTs[][2] = {{1, 1}, {1, 8}, {9, 1}, {9, 2}, {9, 3}, {9, 5}, {9, 8}, {25, 4}, {16, 33}, {1, 15}, {1, 16}, {1, 17}};
  const int Rs[] = {1, 2, 3, 7, 8, 12, 16, 17, 64, 255, 256, 304, 1024};
  for (long M : Ms)
    for (int N : Ns)
      for (auto& k : KTs)
        for (int R : Rs) {
          ufr_igemm_desc d = make(M, N, k[0], k[1]);
          const int rc = ufr_igemm_tail_plan(&d, R, &p);
          CHECK(rc == UFR_OK, "M=%ld N=%d R=%d: rc %d (%s)", M, N, R, rc, ufr_last_error());
          if (rc == UFR_OK) check_plan(d, R, p);
        }
  // the headline: conv3_1's data gradient on the correlation-reach band, 8 pairs of 384 x 1280
  {
    ufr_igemm_desc d = make(21504, 512, 9, 8);
    CHECK(ufr_igemm_tail_plan(&d, 256, &p) == UFR_OK && p.on && p.full_row_tiles == 64 && p.tail_row_tiles == 20 && p.slices == 3 &&
              p.slice_ktiles == 24 && p.workgroups == 496 && p.tail_rows == 5120,
          "headline geometry");
    ufr_igemm_tail_plan_t p0;
    CHECK(ufr_igemm_tail_plan(&d, 0, &p0) == UFR_OK && std::memcmp(&p, &p0, sizeof p) == 0, "resident = 0 is the 256-CU chip");
    // every refused configuration is off
    struct { const char* what; void (*edit)(ufr_igemm_desc&); } off[] = {
        {"two phases", [](ufr_igemm_desc& x) { x.nphase = 2; x.phase[1].ntaps = 9; }},
        {"64-column tiles", [](ufr_igemm_desc& x) { x.Npad = 448; x.N = 448; }},
        {"variant 7", [](ufr_igemm_desc& x) { x.variant = 7; }},
        {"variant 0", [](ufr_igemm_desc& x) { x.variant = 0; }},
        {"three products", [](ufr_igemm_desc& x) { x.products = 3; }},
        {"tickets", [](ufr_igemm_desc& x) { x.tickets = reinterpret_cast<int*>(4096); }},
        {"no_reduce", [](ufr_igemm_desc& x) { x.no_reduce = 1; }},
        {"tail output", [](ufr_igemm_desc& x) { x.tail = reinterpret_cast<float*>(4096); x.tail_n0 = 32; }},
        {"split-K", [](ufr_igemm_desc& x) { x.splitk = 2; }},
        {"no full round", [](ufr_igemm_desc& x) { x.Wr = 256 * 60; }},
        {"whole rounds", [](ufr_igemm_desc& x) { x.Wr = 256 * 128; }},
        {"short reduction", [](ufr_igemm_desc& x) { x.KC = 1; }},
    };
    for (auto& c : off) {
      ufr_igemm_desc e = d;
      c.edit(e);
      CHECK(ufr_igemm_tail_plan(&e, 256, &p) == UFR_OK && !p.on && p.ws_floats == 0, "%s: not off", c.what);
    }
    // arguments refused outright
    CHECK(ufr_igemm_tail_plan(nullptr, 256, &p) == UFR_EINVAL, "null descriptor");
    CHECK(ufr_igemm_tail_plan(&d, 256, nullptr) == UFR_EINVAL, "null plan");
    CHECK(ufr_igemm_tail_plan(&d, -1, &p) == UFR_EINVAL, "negative resident count");
    ufr_igemm_desc e = d;
    e.B = 1 << 15; e.Hr = 1 << 15; e.Wr = 4;
    CHECK(ufr_igemm_tail_plan(&e, 256, &p) == UFR_EINVAL, "2^32 rows");
    e = d;
    e.phase[0].ntaps = UFR_IGEMM_MAX_TAPS + 1;
    CHECK(ufr_igemm_tail_plan(&e, 256, &p) == UFR_EINVAL, "too many taps");
    // the balanced entry with a plan that is on and too little room for its slabs: refused before it asks for a device
    float* ws = reinterpret_cast<float*>(4096);
    CHECK(ufr_igemm_tail_plan(&d, 256, &p) == UFR_OK && p.on, "headline plan");
    CHECK(ufr_igemm_balanced(&d, 256, ws, p.ws_floats - 1, nullptr) == UFR_EINVAL && std::strstr(ufr_last_error(), "workspace"), "small workspace");
    CHECK(ufr_igemm_balanced(&d, 256, nullptr, p.ws_floats, nullptr) == UFR_EINVAL && std::strstr(ufr_last_error(), "workspace"), "null workspace");
  }
  std::printf("%ld plans on, %ld off, %d failures\n", plans_on, plans_off, failures);
  return failures ? 1 : 0;
}
