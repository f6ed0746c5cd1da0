// Stand-alone host program for the argument validation of the figures' entries (csrc/flow_viz.hip): ufr_flow_to_image,
// ufr_eval_blend_gt, ufr_sweep_blend_gt, ufr_viz_ranges, ufr_viz_strip and their two workspace sizes, meant to be built with the host
// side under AddressSanitizer and UBSan (tests/test_figures_cabi_cpu.py: hipcc -Xarch_host -fsanitize=address,undefined) and run
// WITHOUT a GPU: every call here is refused before any HIP call, so no device pointer is dereferenced and no kernel is launched.
// What the sanitizers watch is the host side of the entries: the copy of the 55 x 3 colour wheel out of the caller's array, the walk
// over the placement tables, and the size arithmetic with operands near INT_MAX.
#include <climits>
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

static void expect_long(long got, long want, const char* what) {
  if (got != want) {
    std::printf("FAIL %s: %ld (wanted %ld)\n", what, got, want);
    ++failures;
  }
}

int main() {
  float* f = reinterpret_cast<float*>(4096);
  unsigned char* u8 = reinterpret_cast<unsigned char*>(4096);
  int* di = reinterpret_cast<int*>(4096);
  const long big = 1L << 40;
  const int K = 3, H = 16, W = 32, Hg = 11, Wg = 23;
  // exactly 165 doubles on the heap: a read past the wheel's end is a sanitizer report
  std::vector<double> wheel(55 * 3, 128.0), bad(wheel);
  bad[164] = 255.5;
  std::vector<int> places = {1, 2, 4, 4, 0, 0, 3, 5, 1, 2, 4, 4, 0, 0, 3, 5, 1, 2, 4, 4, 0, 0, 3, 5};
  std::vector<int> far(places), tall(places);
  far[2 * 8 + 1] = INT_MAX;                 // item 2, first frame: x near INT_MAX
  tall[1 * 8 + 6] = INT_MAX;                // item 1, second frame: h near INT_MAX
  std::vector<int> origins = {0, 0, 3, 5, 11, 27}, leaving(origins);
  leaving[4] = INT_MAX;

  // ---- workspace sizes
  expect_long(ufr_flow_to_image_workspace_floats(0), -1, "flow to image workspace: K = 0");
  expect_long(ufr_flow_to_image_workspace_floats(INT_MIN), -1, "flow to image workspace: K = INT_MIN");
  expect_long(ufr_flow_to_image_workspace_floats(INT_MAX), 128L * INT_MAX, "flow to image workspace: K = INT_MAX");
  expect_long(ufr_viz_workspace_floats(-1), -1, "viz workspace: K < 0");
  expect_long(ufr_viz_workspace_floats(INT_MAX), 128L * 8 * INT_MAX, "viz workspace: K = INT_MAX");
  const long ws_f = ufr_flow_to_image_workspace_floats(K), ws_v = ufr_viz_workspace_floats(K);

  // ---- ufr_flow_to_image
  expect(ufr_flow_to_image(nullptr, f, wheel.data(), u8, K, H, W, f, big, nullptr), "null pointer", "flow to image: null flow");
  expect(ufr_flow_to_image(f, nullptr, nullptr, u8, K, H, W, f, big, nullptr), "null pointer", "flow to image: null wheel");
  expect(ufr_flow_to_image(f, f, wheel.data(), nullptr, K, H, W, f, big, nullptr), "null pointer", "flow to image: null out");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, K, H, W, nullptr, big, nullptr), "null pointer", "flow to image: null workspace");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, 0, H, W, f, big, nullptr), "bad shape", "flow to image: K = 0");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, 65536, H, W, f, big, nullptr), "bad shape", "flow to image: K > 65535");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, K, INT_MIN, W, f, big, nullptr), "bad shape", "flow to image: H = INT_MIN");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, K, H, 0, f, big, nullptr), "bad shape", "flow to image: W = 0");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, K, INT_MAX, INT_MAX, f, big, nullptr), "too many pixels", "flow to image: pixels near 2^62");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, K, H, W, f, ws_f - 1, nullptr), "workspace", "flow to image: small workspace");
  expect(ufr_flow_to_image(f, f, wheel.data(), u8, K, H, W, f, -1, nullptr), "workspace", "flow to image: negative workspace");
  expect(ufr_flow_to_image(f, f, bad.data(), u8, K, H, W, f, big, nullptr), "colour wheel entry 164", "flow to image: the wheel's last entry");

  // ---- ufr_eval_blend_gt
  expect(ufr_eval_blend_gt(nullptr, f, f, f, di, places.data(), f, K, H, W, Hg, Wg, 6, 6, 0, nullptr), "null pointer", "eval blend: null gt");
  expect(ufr_eval_blend_gt(f, f, f, f, di, nullptr, f, K, H, W, Hg, Wg, 6, 6, 0, nullptr), "needed on the host", "eval blend: no host table");
  expect(ufr_eval_blend_gt(f, f, f, f, di, places.data(), nullptr, K, H, W, Hg, Wg, 6, 6, 0, nullptr), "null pointer", "eval blend: null g");
  expect(ufr_eval_blend_gt(f, f, f, f, di, places.data(), f, 0, H, W, Hg, Wg, 6, 6, 0, nullptr), "bad shape", "eval blend: K = 0");
  expect(ufr_eval_blend_gt(f, f, f, f, di, places.data(), f, K, H, W, 0, Wg, 6, 6, 0, nullptr), "bad shape", "eval blend: Hg = 0");
  expect(ufr_eval_blend_gt(f, f, f, f, di, places.data(), f, K, H, W, Hg, Wg, INT_MAX, 6, 0, nullptr), "larger than", "eval blend: sh = INT_MAX");
  expect(ufr_eval_blend_gt(f, f, f, f, di, places.data(), f, K, INT_MAX, INT_MAX, Hg, Wg, 6, 6, 0, nullptr), "too many pixels",
         "eval blend: pixels near 2^62");
  expect(ufr_eval_blend_gt(f, f, f, f, di, places.data(), f, K, H, W, Hg, Wg, 6, 6, 2, nullptr), "ignore_mask_flow", "eval blend: flag 2");
  expect(ufr_eval_blend_gt(f, f, f, f, di, far.data(), f, K, H, W, Hg, Wg, 6, 6, 0, nullptr), "leaves the 16x32 frame", "eval blend: x near INT_MAX");
  expect(ufr_eval_blend_gt(f, f, f, f, di, tall.data(), f, K, H, W, Hg, Wg, 6, 6, 0, nullptr), "does not fit", "eval blend: h near INT_MAX");

  // ---- ufr_sweep_blend_gt
  expect(ufr_sweep_blend_gt(f, nullptr, di, origins.data(), f, K, H, W, Hg, Wg, 5, 5, 1, nullptr), "null pointer", "sweep blend: null mask");
  expect(ufr_sweep_blend_gt(f, f, di, nullptr, f, K, H, W, Hg, Wg, 5, 5, 1, nullptr), "null pointer", "sweep blend: no host origins");
  expect(ufr_sweep_blend_gt(f, f, di, origins.data(), f, INT_MIN, H, W, Hg, Wg, 5, 5, 1, nullptr), "bad shape", "sweep blend: K = INT_MIN");
  expect(ufr_sweep_blend_gt(f, f, di, origins.data(), f, K, H, W, Hg, Wg, 0, 5, 1, nullptr), "bad shape", "sweep blend: ph = 0");
  expect(ufr_sweep_blend_gt(f, f, di, origins.data(), f, K, H, W, Hg, Wg, 5, INT_MAX, 1, nullptr), "larger than", "sweep blend: pw = INT_MAX");
  expect(ufr_sweep_blend_gt(f, f, di, origins.data(), f, K, H, W, Hg, Wg, 5, 5, -1, nullptr), "valid_in_patch", "sweep blend: flag -1");
  expect(ufr_sweep_blend_gt(f, f, di, leaving.data(), f, K, H, W, Hg, Wg, 5, 5, 1, nullptr), "leaves the 16x32 frame", "sweep blend: y near INT_MAX");

  // ---- ufr_viz_ranges, ufr_viz_strip
  expect(ufr_viz_ranges(f, f, f, f, nullptr, K, H, W, Hg, Wg, f, big, f, nullptr), "null pointer", "ranges: null g");
  expect(ufr_viz_ranges(f, f, f, f, f, K, H, W, Hg, Wg, f, big, nullptr, nullptr), "null pointer", "ranges: null record");
  expect(ufr_viz_ranges(f, f, f, f, f, 0, H, W, Hg, Wg, f, big, f, nullptr), "bad shape", "ranges: K = 0");
  expect(ufr_viz_ranges(f, f, f, f, f, K, H, INT_MIN, Hg, Wg, f, big, f, nullptr), "bad shape", "ranges: W = INT_MIN");
  expect(ufr_viz_ranges(f, f, f, f, f, K, H, W, 0, Wg, f, big, f, nullptr), "without its sizes", "ranges: Hg = 0");
  expect(ufr_viz_ranges(f, f, f, f, f, K, H, W, Hg, INT_MIN, f, big, f, nullptr), "without its sizes", "ranges: Wg = INT_MIN");
  expect(ufr_viz_ranges(f, f, f, f, f, K, INT_MAX, INT_MAX, Hg, Wg, f, big, f, nullptr), "too many pixels", "ranges: pixels near 2^62");
  expect(ufr_viz_ranges(f, f, f, f, f, K, H, W, Hg, Wg, f, ws_v - 1, f, nullptr), "workspace", "ranges: small workspace");
  expect(ufr_viz_strip(f, f, f, f, f, nullptr, wheel.data(), u8, K, H, W, Hg, Wg, nullptr), "null pointer", "strip: null record");
  expect(ufr_viz_strip(f, f, f, f, f, f, nullptr, u8, K, H, W, Hg, Wg, nullptr), "null pointer", "strip: null wheel");
  expect(ufr_viz_strip(f, f, f, f, f, f, wheel.data(), nullptr, K, H, W, Hg, Wg, nullptr), "null pointer", "strip: null out");
  expect(ufr_viz_strip(f, f, f, f, f, f, wheel.data(), u8, 65536, H, W, Hg, Wg, nullptr), "bad shape", "strip: K > 65535");
  expect(ufr_viz_strip(f, f, f, f, f, f, wheel.data(), u8, K, H, W, Hg, 0, nullptr), "without its sizes", "strip: Wg = 0");
  expect(ufr_viz_strip(f, f, f, f, f, f, wheel.data(), u8, K, 1 << 13, 1 << 13, Hg, Wg, nullptr), "too many pixels", "strip: 2^26 pixels");
  expect(ufr_viz_strip(f, f, f, f, f, f, bad.data(), u8, K, H, W, Hg, Wg, nullptr), "colour wheel entry 164", "strip: the wheel's last entry");
  std::printf(failures ? "%d failure(s)\n" : "figures args: all refused, %d failures\n", failures);
  return failures ? 1 : 0;
}
