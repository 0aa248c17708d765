// Host-side check of the layer backward's GEMM table (csrc/layer.hip: BwdGemms, the carvers that size a workspace from it,
// xp_debug_layer_bwd_gemms), as a stand-alone program for a sanitizer build -- it needs no GPU: the four workspace queries and the
// table query launch nothing, and the backward calls below are refused before their first launch.
//
//   cd xpretrain_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -x hip *.hip common.cpp ../../tools/layer_table_host_check.cpp -o /tmp/layer_table_host_check && /tmp/layer_table_host_check
//
// The dims are those of tests/golden/layer_gemm_table_workspace_bytes.json (tests/test_layer_gemm_table_cpu.py::SHAPES), both
// dtypes, both activations, CU budgets 256 and 128.  Exit status 0 and "ok" on the last line: the table is consistent with the
// planning queries and with the workspace sizes, and the sanitizers had nothing to report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../include/xpretrain_hip.h"

static int failures = 0;
static void expect(bool ok, const char* what, const char* shape, int dt, int act, int budget) {
  if (ok) return;
  printf("FAIL  %s  (%s dtype %d act %d budget %d): %s\n", what, shape, dt, act, budget, xp_last_error());
  ++failures;
}

struct Shape { const char* name; int64_t B, S, D, Dff, heads, M, N, L; };      // M == 0: the causal text layer
static const Shape SHAPES[] = {{"step_video", 8, 2356, 768, 3072, 12, 4, 12, 196}, {"step_text", 8, 32, 512, 2048, 8, 0, 1, 32},
                               {"listed_8240", 2, 4120, 768, 3072, 12, 4, 21, 196}, {"small_video", 4, 10, 128, 512, 2, 2, 2, 4},
                               {"small_text", 3, 50, 256, 1024, 4, 0, 1, 50}};

int main() {
  int checked = 0;
  for (int budget : {256, 128}) {
    xp_set_cu_budget(budget);
    for (const Shape& s : SHAPES)
      for (int dt : {XP_BF16, XP_F32})
        for (int act : {XP_ACT_QUICK_GELU, XP_ACT_GELU}) {
          XpLayerDims d;
          memset(&d, 0, sizeof d);
          d.rows = s.B * s.S; d.D = s.D; d.Dff = s.Dff; d.B = s.B; d.S = s.S; d.heads = s.heads; d.M = s.M; d.N = s.N; d.L = s.L;
          d.attn_mode = s.M ? XP_ATTN_PROXY : XP_ATTN_CAUSAL; d.dtype = dt; d.q_scale = 0.125f; d.ln_eps = 1e-5f; d.act = act;
          auto ex = [&](bool ok, const char* what) { expect(ok, what, s.name, dt, act, budget); };
          ex(xp_encoder_layer_fwd_workspace_bytes(&d) > 256 && xp_encoder_layer_bwd_workspace_bytes(&d) > 256, "dense workspace queries");
          for (int pooled = 0; pooled <= (s.M ? 1 : 0); ++pooled) {
            XpGemmDesc t[XP_LAYER_GEMM_MAX + 1];
            memset(t, 0x5a, sizeof t);                                       // (a write past the count shows as a changed byte)
            const int want = pooled ? XP_LAYER_GEMM_POOLED_COUNT : XP_LAYER_GEMM_DENSE_COUNT;
            const int n = xp_debug_layer_bwd_gemms(&d, pooled, t, XP_LAYER_GEMM_MAX);
            ex(n == want, "row count");
            XpGemmDesc pat;
            memset(&pat, 0x5a, sizeof pat);
            for (int i = want; i <= XP_LAYER_GEMM_MAX; ++i) ex(!memcmp(&t[i], &pat, sizeof pat), "nothing written past the count");
            size_t slabs = 0;
            for (int i = 0; i < n && i < want; ++i) {
              const XpGemmDesc& g = t[i];
              ex(!g.A && !g.B && !g.C && !g.bias && !g.aux && !g.m_tiles && !g.k_tiles && g.M > 0 && g.N > 0 && g.K > 0, "a row has no operands");
              XpGemmPlanInfo p;
              ex(xp_debug_gemm_plan(&g, &p) == XP_OK && p.split == g.split_k, "a row plans at its split");
              if (g.a_kstrided && g.b_kstrided) {                            // a weight gradient: one of the two rules, slabs for either
                const int a = xp_gemm_auto_split(&g), b = xp_gemm_auto_split_slack(&g), most = a > b ? a : b;
                ex(g.split_k == (a > 1 ? a : 1) || g.split_k == (b > 1 ? b : 1), "a weight gradient's split is a planned one");
                const size_t bytes = most > 1 ? (size_t)most * g.M * g.N * 4 : 0;
                if (bytes > slabs) slabs = bytes;
              }
              if (i == XP_LAYER_GEMM_DPRE)
                ex(g.resid && (g.colsum_partials != nullptr) == (!pooled && xp_gemm_colsum_rows(&g) > 0), "dpre: resid, fused sums where planned");
            }
            const size_t ws = pooled ? xp_encoder_layer_pooled_bwd_workspace_bytes(&d) : xp_encoder_layer_bwd_workspace_bytes(&d);
            ex(ws > slabs + 256, "the workspace holds the slabs of the table");
            ex(xp_debug_layer_bwd_gemms(&d, pooled, t, want - 1) == XP_ERR_ARG, "a short output array is refused");
            ++checked;
          }
          if (s.M) ex(xp_encoder_layer_pooled_fwd_workspace_bytes(&d) > 256, "pooled forward workspace query");
          // the backward calls themselves, up to their workspace check: the table is built, the carver walks it, nothing is launched
          alignas(16) static char buf[256];
          XpLayerBwd a;
          memset(&a, 0, sizeof a);
          a.dims = d;
          a.x = a.h1 = a.qkv = a.attn_o = a.x2 = a.h2 = a.pre = a.act = a.Wqkv = a.Wo = a.W1 = a.W2 = a.dx3 = buf;
          a.ln1_w = a.ln2_w = a.mean1 = a.rstd1 = a.mean2 = a.rstd2 = a.stats = (const float*)buf;
          a.dx = buf; a.workspace = buf; a.workspace_bytes = sizeof buf;
          ex(xp_encoder_layer_bwd(&a, nullptr) == XP_ERR_ARG && strstr(xp_last_error(), "workspace too small"), "dense backward refuses a short workspace");
        }
  }
  XpGemmDesc t[XP_LAYER_GEMM_MAX];
  expect(xp_debug_layer_bwd_gemms(nullptr, 0, t, XP_LAYER_GEMM_MAX) == XP_ERR_ARG, "null dims are refused", "-", 0, 0, 0);
  printf("%d tables checked\n", checked);
  printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
  return failures != 0;
}
