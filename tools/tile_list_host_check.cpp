// Host-side check of the tile-list planning and validation in xp_gemm (csrc/gemm.hip), as a stand-alone program for a
// sanitizer build -- it needs no GPU: every call below is answered (planned, or refused by a check) before anything is launched;
// no call here is a valid launch.
//
//   cd xpretrain_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -x hip gemm.hip gemm256.hip common.cpp ../../tools/tile_list_host_check.cpp -o /tmp/tile_list_host_check && /tmp/tile_list_host_check
//
// Exit status 0 and "ok" on the last line: every refusal came back as an error code with its message, the plan of a listed
// call is the dense call's, and the sanitizers had nothing to report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/xpretrain_hip.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
  printf("%s  %s\n", ok ? "pass" : "FAIL", what);
  failures += !ok;
}
static bool refused(const XpGemmDesc& d, const char* needle) {
  const int rc = xp_gemm(&d, nullptr);
  const char* msg = xp_last_error();
  return rc != 0 && msg && strstr(msg, needle);
}

int main() {
  alignas(16) static char a[64], b[64], c[64];      // never dereferenced: every call ends before a launch
  std::vector<int32_t> begin = {0, 2, 4, 6};
  alignas(4) static int32_t dev_list[16];           // stands for a device array: the host never reads it

  // the dX form: M = 31 * 256 + 40, N = 768, K = 256 (32 x 3 tiles: a 256-wide plan)
  XpGemmDesc dx;
  memset(&dx, 0, sizeof dx);
  dx.A = a; dx.B = b; dx.C = c; dx.M = 31 * 256 + 40; dx.N = 768; dx.K = 256;
  dx.lda = 256; dx.ldb = 768; dx.ldc = 768; dx.ldr = 768; dx.ldaux = 768; dx.b_kstrided = 1;
  dx.in_dtype = XP_BF16; dx.out_dtype = XP_BF16; dx.split_k = 1; dx.scale = 1.f;
  XpGemmPlanInfo dense, listed;
  expect(xp_debug_gemm_plan(&dx, &dense) == 0 && dense.family == XP_GEMM_FAMILY_256 && dense.tiles_m == 32, "dX form plans 256-wide, 32 row tiles");

  XpGemmDesc d = dx;
  d.m_tiles = dev_list; d.n_m_tiles = 3;
  expect(xp_debug_gemm_plan(&d, &listed) == 0 && listed.family == dense.family && listed.tiles_m == dense.tiles_m &&
         listed.tiles_n == dense.tiles_n && listed.group_n == dense.group_n && listed.k_per_split == dense.k_per_split &&
         listed.epi_impl == dense.epi_impl && listed.colsum_rows == dense.colsum_rows, "a listed call is planned as the dense call");
  d.n_m_tiles = 33;
  expect(refused(d, "m_tiles needs"), "more row tiles than the problem has");
  d.n_m_tiles = 0;
  expect(refused(d, "m_tiles needs"), "an empty row-tile list");
  d = dx; d.n_m_tiles = 2;
  expect(refused(d, "m_tiles needs"), "a count without a list");
  d = dx; d.m_tiles = dev_list; d.n_m_tiles = 1; d.M = 1024;
  expect(refused(d, "256-wide-family plan"), "a plan of the 128-row family");
  d = dx; d.m_tiles = dev_list; d.n_m_tiles = 1; d.k_tiles = dev_list; d.k_tile_begin = dev_list; d.k_tile_begin_host = begin.data();
  expect(refused(d, "different operand layouts"), "both kinds of list");
  d = dx; d.k_tiles = dev_list; d.k_tile_begin = dev_list; d.k_tile_begin_host = begin.data();
  expect(refused(d, "dW form"), "k-tile lists on the dX form");

  // the dW form: dW[3072, 768] over K = 750 rows, split 3 (slabs of 4, 4 and 4 k-tiles, the last one partial)
  XpGemmDesc dw;
  memset(&dw, 0, sizeof dw);
  dw.A = a; dw.B = b; dw.C = c; dw.M = 3072; dw.N = 768; dw.K = 750;
  dw.lda = 3072; dw.ldb = 768; dw.ldc = 768; dw.ldr = 768; dw.ldaux = 768; dw.a_kstrided = dw.b_kstrided = 1;
  dw.in_dtype = XP_BF16; dw.out_dtype = XP_F32; dw.split_k = 3; dw.scale = 1.f;
  expect(xp_debug_gemm_plan(&dw, &dense) == 0 && dense.family == XP_GEMM_FAMILY_256 && dense.split == 3 && dense.k_per_split == 256,
         "dW form plans 256-wide, 3 slabs of 256 rows");
  d = dw; d.m_tiles = dev_list; d.n_m_tiles = 1;
  expect(refused(d, "dX form"), "a row-tile list on the dW form");
  d = dw; d.k_tiles = dev_list; d.k_tile_begin = dev_list;
  expect(refused(d, "k_tile_begin_host"), "no host copy of k_tile_begin");
  std::vector<int32_t> shallow = {0, 2, 3, 5}, deep = {0, 4, 8, 13}, negative = {-1, 2, 4, 6};
  d.k_tile_begin_host = shallow.data();
  expect(refused(d, "needs 2"), "a slab below the pipeline depth");
  d.k_tile_begin_host = deep.data();
  expect(refused(d, "needs 2"), "a slab that lists more k-tiles than it has");
  d.k_tile_begin_host = negative.data();
  expect(refused(d, "negative"), "a negative first offset");
  printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
  return failures != 0;
}
