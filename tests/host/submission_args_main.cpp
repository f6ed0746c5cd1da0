// Stand-alone host program for the argument validation of ufr_forward_interpolate / ufr_forward_interpolate_sliced /
// ufr_flow_encode (csrc/submission.hip), meant to be built with the host side under AddressSanitizer and UBSan
// (tests/test_submission_cpu.py: hipcc -Xarch_host -fsanitize=address,undefined) and run WITHOUT a GPU: every call here is refused
// before any HIP call, so no pointer is dereferenced and no kernel is launched.  What the sanitizers watch is the host arithmetic
// of the entries: the pixel counts and the crop's extent, with operands near INT_MAX.
#include <climits>
#include <cstdio>
#include <cstring>

#include "../../include/ufr_hip.h"

static int failures = 0;

static void expect(int rc, const char* needle, const char* what) {
  const char* msg = ufr_last_error();
  if (rc != UFR_EINVAL || std::strstr(msg, needle) == nullptr) {
    std::printf("FAIL %s: rc=%d message='%s' (wanted '%s')\n", what, rc, msg, needle);
    ++failures;
  }
}

int main() {
  float* f = reinterpret_cast<float*>(4096);
  void* o = reinterpret_cast<void*>(8192);
  const int B = 2, K = 3, H = 5, W = 7, top = 1, left = 0, Hp = 8, Wp = 8;

  // ---- ufr_forward_interpolate, ufr_forward_interpolate_sliced
  expect(ufr_forward_interpolate(nullptr, f, B, H, W, nullptr), "null pointer", "interpolate: null flow");
  expect(ufr_forward_interpolate(f, nullptr, B, H, W, nullptr), "null pointer", "interpolate: null out");
  expect(ufr_forward_interpolate(f, f, 0, H, W, nullptr), "bad shape", "interpolate: B = 0");
  expect(ufr_forward_interpolate(f, f, INT_MIN, H, W, nullptr), "bad shape", "interpolate: B = INT_MIN");
  expect(ufr_forward_interpolate(f, f, 65536, H, W, nullptr), "bad shape", "interpolate: B > 65535");
  expect(ufr_forward_interpolate(f, f, B, 0, W, nullptr), "bad shape", "interpolate: H = 0");
  expect(ufr_forward_interpolate(f, f, B, H, -7, nullptr), "bad shape", "interpolate: W < 0");
  expect(ufr_forward_interpolate(f, f, B, INT_MAX, INT_MAX, nullptr), "too many pixels", "interpolate: pixels near 2^62");
  expect(ufr_forward_interpolate(f, f, B, 1 << 15, 1 << 14, nullptr), "too many pixels", "interpolate: 2^29 pixels");
  expect(ufr_forward_interpolate_sliced(nullptr, f, B, H, W, 4, nullptr), "null pointer", "sliced: null flow");
  expect(ufr_forward_interpolate_sliced(f, f, B, H, W, 0, nullptr), "slices 0", "sliced: no slices");
  expect(ufr_forward_interpolate_sliced(f, f, B, H, W, 8, nullptr), "slices 8", "sliced: 8 slices");
  expect(ufr_forward_interpolate_sliced(f, f, B, H, W, INT_MIN, nullptr), "slices", "sliced: INT_MIN slices");
  expect(ufr_forward_interpolate_sliced(f, f, B, INT_MAX, W, 16, nullptr), "too many pixels", "sliced: rows near INT_MAX");

  // ---- ufr_flow_encode
  expect(ufr_flow_encode(nullptr, o, K, Hp, Wp, top, left, H, W, 0, nullptr), "null pointer", "encode: null pred");
  expect(ufr_flow_encode(f, nullptr, K, Hp, Wp, top, left, H, W, 1, nullptr), "null pointer", "encode: null out");
  expect(ufr_flow_encode(f, o, 0, Hp, Wp, top, left, H, W, 0, nullptr), "bad shape", "encode: K = 0");
  expect(ufr_flow_encode(f, o, INT_MIN, Hp, Wp, top, left, H, W, 0, nullptr), "bad shape", "encode: K = INT_MIN");
  expect(ufr_flow_encode(f, o, K, 0, Wp, top, left, H, W, 0, nullptr), "bad shape", "encode: Hp = 0");
  expect(ufr_flow_encode(f, o, K, Hp, -1, top, left, H, W, 0, nullptr), "bad shape", "encode: Wp < 0");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, top, left, 0, W, 0, nullptr), "bad shape", "encode: H = 0");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, top, left, H, INT_MIN, 0, nullptr), "bad shape", "encode: W = INT_MIN");
  expect(ufr_flow_encode(f, o, K, INT_MAX, INT_MAX, top, left, INT_MAX, INT_MAX, 0, nullptr), "too many pixels", "encode: pixels near 2^62");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, -1, left, H, W, 0, nullptr), "negative pad", "encode: top < 0");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, top, INT_MIN, H, W, 0, nullptr), "negative pad", "encode: left = INT_MIN");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, 4, left, H, W, 0, nullptr), "leaves the padded frame", "encode: rows leave");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, top, 2, H, W, 1, nullptr), "leaves the padded frame", "encode: columns leave");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, INT_MAX, INT_MAX, H, W, 0, nullptr), "leaves the padded frame", "encode: offsets near INT_MAX");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, top, left, H, W, 2, nullptr), "mode 2", "encode: mode 2");
  expect(ufr_flow_encode(f, o, K, Hp, Wp, top, left, H, W, -1, nullptr), "mode -1", "encode: mode -1");
  std::printf(failures ? "%d failure(s)\n" : "submission args: all refused, %d failures\n", failures);
  return failures ? 1 : 0;
}
