// Stand-alone host program for the argument validation of ufr_validation_pad / ufr_validation_metrics /
// ufr_validation_metrics_workspace_doubles (csrc/validation.hip), meant to be built with the host side under AddressSanitizer and
// UBSan (tests/test_validation_host_cpu.py: hipcc -Xarch_host -fsanitize=address,undefined) and run WITHOUT a GPU: every call here
// is refused before any HIP call, so no pointer is dereferenced and no kernel is launched.  What the sanitizers watch is the host
// arithmetic of the entries: the padded sizes, the crop's extent, the row range and the workspace size, with operands near INT_MAX.
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

static void expect_long(long got, long want, const char* what) {
  if (got != want) {
    std::printf("FAIL %s: %ld (wanted %ld)\n", what, got, want);
    ++failures;
  }
}

int main() {
  float* f = reinterpret_cast<float*>(4096);
  double* d = reinterpret_cast<double*>(4096);
  const long big = 1L << 40;
  const int K = 3, H = 5, W = 7, top = 1, bottom = 2, left = 0, right = 1, Hp = 8, Wp = 8;

  // ---- ufr_validation_pad
  expect(ufr_validation_pad(nullptr, f, f, f, K, H, W, top, bottom, left, right, 0, nullptr), "null pointer", "pad: null image1");
  expect(ufr_validation_pad(f, nullptr, f, f, K, H, W, top, bottom, left, right, 0, nullptr), "null pointer", "pad: null image2");
  expect(ufr_validation_pad(f, f, nullptr, f, K, H, W, top, bottom, left, right, 1, nullptr), "null pointer", "pad: null out1");
  expect(ufr_validation_pad(f, f, f, nullptr, K, H, W, top, bottom, left, right, 1, nullptr), "null pointer", "pad: null out2");
  expect(ufr_validation_pad(f, f, f, f, 0, H, W, top, bottom, left, right, 0, nullptr), "bad shape", "pad: K = 0");
  expect(ufr_validation_pad(f, f, f, f, INT_MIN, H, W, top, bottom, left, right, 0, nullptr), "bad shape", "pad: K = INT_MIN");
  expect(ufr_validation_pad(f, f, f, f, K, 0, W, top, bottom, left, right, 0, nullptr), "bad shape", "pad: H = 0");
  expect(ufr_validation_pad(f, f, f, f, K, H, -7, top, bottom, left, right, 0, nullptr), "bad shape", "pad: W < 0");
  expect(ufr_validation_pad(f, f, f, f, K, H, W, -1, bottom, left, right, 0, nullptr), "negative pad", "pad: top < 0");
  expect(ufr_validation_pad(f, f, f, f, K, H, W, top, INT_MIN, left, right, 0, nullptr), "negative pad", "pad: bottom = INT_MIN");
  expect(ufr_validation_pad(f, f, f, f, K, H, W, top, bottom, -3, right, 0, nullptr), "negative pad", "pad: left < 0");
  expect(ufr_validation_pad(f, f, f, f, K, H, W, top, bottom, left, -1, 0, nullptr), "negative pad", "pad: right < 0");
  expect(ufr_validation_pad(f, f, f, f, K, INT_MAX, W, INT_MAX, INT_MAX, left, right, 0, nullptr), "too large", "pad: rows near INT_MAX");
  expect(ufr_validation_pad(f, f, f, f, K, H, INT_MAX, top, bottom, INT_MAX, INT_MAX, 0, nullptr), "too large", "pad: columns near INT_MAX");
  expect(ufr_validation_pad(f, f, f, f, INT_MAX, (1 << 20) - 8, (1 << 20) - 8, 1, 1, 1, 1, 0, nullptr), "too many pixels", "pad: pixels");

  // ---- ufr_validation_metrics_workspace_doubles
  expect_long(ufr_validation_metrics_workspace_doubles(0, H, W), -1, "workspace: K = 0");
  expect_long(ufr_validation_metrics_workspace_doubles(K, 0, W), -1, "workspace: H = 0");
  expect_long(ufr_validation_metrics_workspace_doubles(K, H, -1), -1, "workspace: W < 0");
  expect_long(ufr_validation_metrics_workspace_doubles(K, INT_MAX, INT_MAX), -1, "workspace: pixels near 2^62");
  expect_long(ufr_validation_metrics_workspace_doubles(1, H, W), 1L * UFR_VALIDATION_COLS, "workspace: one workgroup");
  expect_long(ufr_validation_metrics_workspace_doubles(K, 125, 187), 3L * 92 * UFR_VALIDATION_COLS, "workspace: 92 workgroups per item");
  expect_long(ufr_validation_metrics_workspace_doubles(K, 376, 1242), 3L * 128 * UFR_VALIDATION_COLS, "workspace: the cap of 128");
  const long ws = ufr_validation_metrics_workspace_doubles(K, H, W);

  // ---- ufr_validation_metrics
  expect(ufr_validation_metrics(nullptr, f, f, K, Hp, Wp, top, left, H, W, 0, d, big, d, 0, K, nullptr), "null pointer", "metrics: null pred");
  expect(ufr_validation_metrics(f, nullptr, f, K, Hp, Wp, top, left, H, W, 0, d, big, d, 0, K, nullptr), "null pointer", "metrics: null gt");
  expect(ufr_validation_metrics(f, f, nullptr, K, Hp, Wp, top, left, H, W, 0, nullptr, big, d, 0, K, nullptr), "null pointer", "metrics: null ws");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 0, d, big, nullptr, 0, K, nullptr), "null pointer", "metrics: null out");
  expect(ufr_validation_metrics(f, f, f, 0, Hp, Wp, top, left, H, W, 0, d, big, d, 0, K, nullptr), "bad shape", "metrics: K = 0");
  expect(ufr_validation_metrics(f, f, f, 65536, Hp, Wp, top, left, H, W, 0, d, big, d, 0, 65536, nullptr), "bad shape", "metrics: K > 65535");
  expect(ufr_validation_metrics(f, f, f, K, 0, Wp, top, left, H, W, 0, d, big, d, 0, K, nullptr), "bad shape", "metrics: Hp = 0");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, INT_MIN, 0, d, big, d, 0, K, nullptr), "bad shape", "metrics: W = INT_MIN");
  expect(ufr_validation_metrics(f, f, f, K, INT_MAX, INT_MAX, top, left, INT_MAX, INT_MAX, 0, d, big, d, 0, K, nullptr), "too many pixels",
         "metrics: pixels near 2^62");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, -1, left, H, W, 0, d, big, d, 0, K, nullptr), "negative pad", "metrics: top < 0");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, INT_MIN, H, W, 0, d, big, d, 0, K, nullptr), "negative pad", "metrics: left = INT_MIN");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, 4, left, H, W, 0, d, big, d, 0, K, nullptr), "leaves the padded frame", "metrics: rows leave");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, 2, H, W, 0, d, big, d, 0, K, nullptr), "leaves the padded frame", "metrics: columns leave");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, INT_MAX, INT_MAX, H, W, 0, d, big, d, 0, K, nullptr), "leaves the padded frame",
         "metrics: offsets near INT_MAX");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 3, d, big, d, 0, K, nullptr), "mode", "metrics: mode 3");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, -1, d, big, d, 0, K, nullptr), "mode", "metrics: mode -1");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 0, d, big, d, 1, K, nullptr), "leave the result buffer", "metrics: row0 + K > rows");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 0, d, big, d, -1, K, nullptr), "leave the result buffer", "metrics: row0 < 0");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 0, d, big, d, INT_MAX, INT_MAX, nullptr), "leave the result buffer",
         "metrics: row0 near INT_MAX");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 0, d, big, d, 0, 0, nullptr), "leave the result buffer", "metrics: no rows");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 0, d, ws - 1, d, 0, K, nullptr), "workspace", "metrics: small workspace");
  expect(ufr_validation_metrics(f, f, f, K, Hp, Wp, top, left, H, W, 0, d, -5, d, 0, K, nullptr), "workspace", "metrics: negative workspace");
  std::printf(failures ? "%d failure(s)\n" : "validation args: all refused, %d failures\n", failures);
  return failures ? 1 : 0;
}
