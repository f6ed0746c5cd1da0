// Stand-alone host program for the argument validation of ufr_feature_stats / ufr_feature_stats_workspace_doubles
// (csrc/feature_stats.hip), meant to be built with the host side under AddressSanitizer and UBSan
// (tests/test_feature_stats_host_cpu.py: hipcc -Xarch_host -fsanitize=address,undefined) and run WITHOUT a GPU: every call here is
// refused before any HIP call, so no pointer is dereferenced and no kernel is launched.  What the sanitizers watch is the host
// arithmetic of the entry: the walk over the caller's table, the extents it computes, and the by-value kernel-argument table it
// fills (UFR_FEATURE_STATS_MAX_SEGS slots) up to the point of refusal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/ufr_hip.h"

static int failures = 0;

static void expect(int rc, const char* needle, const char* what) {
  const char* msg = ufr_last_error();
  if (rc != UFR_EINVAL || std::strstr(msg, needle) == nullptr) {
    std::printf("FAIL %s: rc=%d message='%s' (wanted '%s')\n", what, rc, msg, needle);
    ++failures;
  }
}

static ufr_feature_stats_seg good() {
  ufr_feature_stats_seg s;
  std::memset(&s, 0, sizeof s);
  s.src = reinterpret_cast<const void*>(4096);
  s.pixels = 48L * 160;
  s.images = 2;
  s.B = 2;
  s.channels = 13 * 32;
  s.plane_stride = 13L * 2 * 48 * 160 * 32;
  return s;
}

int main() {
  double* p = reinterpret_cast<double*>(4096);
  const long big = 1L << 40;
  ufr_feature_stats_seg s = good();
  expect(ufr_feature_stats(nullptr, 1, p, big, p, 2, 416, 416, nullptr), "null pointer", "null table");
  expect(ufr_feature_stats(&s, 1, nullptr, big, p, 2, 416, 416, nullptr), "null pointer", "null workspace");
  expect(ufr_feature_stats(&s, 1, p, big, nullptr, 2, 416, 416, nullptr), "null pointer", "null result");
  expect(ufr_feature_stats(&s, 0, p, big, p, 2, 416, 416, nullptr), "segments", "no segment");
  expect(ufr_feature_stats(&s, UFR_FEATURE_STATS_MAX_SEGS + 1, p, big, p, 2, 416, 416, nullptr), "segments", "too many segments");
  expect(ufr_feature_stats(&s, -5, p, big, p, 2, 416, 416, nullptr), "segments", "negative count");
  struct { const char* what; const char* needle; void (*edit)(ufr_feature_stats_seg&); } bad[] = {
      {"null planes", "null pointer", [](ufr_feature_stats_seg& x) { x.src = nullptr; }},
      {"kind", "kind", [](ufr_feature_stats_seg& x) { x.kind = 7; }},
      {"no pixels", "bad shape", [](ufr_feature_stats_seg& x) { x.pixels = 0; }},
      {"huge pixels", "bad shape", [](ufr_feature_stats_seg& x) { x.pixels = 1L << 40; }},
      {"negative chunk0", "bad shape", [](ufr_feature_stats_seg& x) { x.chunk0 = -1; }},
      {"huge chunk0", "bad shape", [](ufr_feature_stats_seg& x) { x.chunk0 = 0x7fffffff; }},
      {"huge channels", "bad shape", [](ufr_feature_stats_seg& x) { x.channels = 0x7fffffff; }},
      {"huge images", "bad shape", [](ufr_feature_stats_seg& x) { x.images = 0x7fffffff; }},
      {"image range", "leave its buffer", [](ufr_feature_stats_seg& x) { x.image0 = 0x7fffffff; }},
      {"chunk range", "leave the planes operand (13 chunks per plane)", [](ufr_feature_stats_seg& x) { x.channels = 14 * 32; }},
      {"chunk offset", "leave the planes operand", [](ufr_feature_stats_seg& x) { x.chunk0 = 3; x.channels = 11 * 32; }},
      {"alignment", "16-byte aligned", [](ufr_feature_stats_seg& x) { x.src = reinterpret_cast<const void*>(4104); }},
      {"negative slope", "unleaky", [](ufr_feature_stats_seg& x) { x.unleaky = -1.0; }},
      {"nan slope", "unleaky", [](ufr_feature_stats_seg& x) { x.unleaky = std::nan(""); }},
      {"nchw channels", "leave the tensor", [](ufr_feature_stats_seg& x) { x.kind = 1; x.plane_stride = 2L * 2 * 48 * 160; x.chunk0 = 1; x.channels = 2; }},
      {"negative column", "column", [](ufr_feature_stats_seg& x) { x.out_col = -1; }},
      {"column range", "leave the result matrix", [](ufr_feature_stats_seg& x) { x.out_col = 1; }},
      {"huge column", "leave the result matrix", [](ufr_feature_stats_seg& x) { x.out_col = 0x7fffffffffffff00L; }},
  };
  for (auto& b : bad) {
    ufr_feature_stats_seg x = good();
    b.edit(x);
    expect(ufr_feature_stats(&x, 1, p, big, p, 2, 416, 416, nullptr), b.needle, b.what);
    if (std::strcmp(b.needle, "leave the result matrix") != 0 && ufr_feature_stats_workspace_doubles(&x, 1) != -1) {
      std::printf("FAIL %s: the workspace query accepted the table\n", b.what);
      ++failures;
    }
  }
  expect(ufr_feature_stats(&s, 1, p, big, p, 1, 416, 416, nullptr), "rows", "rows");
  expect(ufr_feature_stats(&s, 1, p, big, p, 2, 416, 400, nullptr), "row stride", "stride");
  // a full table: every slot of the by-value argument table is filled before the workspace is found too small
  std::vector<ufr_feature_stats_seg> full(UFR_FEATURE_STATS_MAX_SEGS, good());
  for (int i = 0; i < UFR_FEATURE_STATS_MAX_SEGS; ++i) full[i].out_col = 0;
  const long need = ufr_feature_stats_workspace_doubles(full.data(), UFR_FEATURE_STATS_MAX_SEGS);
  if (need != 32L * 2 * 13 * 4 * 32) {
    std::printf("FAIL workspace of a full table: %ld\n", need);
    ++failures;
  }
  expect(ufr_feature_stats(full.data(), UFR_FEATURE_STATS_MAX_SEGS, p, need - 1, p, 2, 416, 416, nullptr), "workspace", "small workspace");
  // the last slot bad: the 31 before it are walked first
  full.back().channels = 14 * 32;
  expect(ufr_feature_stats(full.data(), UFR_FEATURE_STATS_MAX_SEGS, p, big, p, 2, 416, 416, nullptr), "segment 31", "last slot");
  std::printf(failures ? "%d failure(s)\n" : "feature stats validation: all refused, %d failures\n", failures);
  return failures ? 1 : 0;
}
