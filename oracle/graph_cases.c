/* oracle/graph_cases.c -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_graph_nodes.py,
 * tests/test_graph_cases_cpu.py).
 *
 * Per-node parity of libvsim_hip.so's graph executor (vsim_graph_compute_rc, graph.cpp) with the
 * reference's own executor: every case builds a small ggml graph with the ggml API alone, runs
 * ggml_graph_compute on it, restores memory, runs vsim_graph_compute_rc on the same graph object
 * and compares the checked tensors bit for bit.  Linked against the reference's ggml.o (compiled
 * in place by oracle/Makefile) and libvsim_hip.so; our own code, nothing of the reference's.
 *
 *   graph_cases --list
 *   graph_cases NAME --threads T                                  reference vs device (needs a GPU)
 *   graph_cases NAME --threads T --ref-only                       reference alone: FNV-1a hashes
 *   graph_cases NAME --threads T --against-threads U --ref-only   reference at T vs reference at U,
 *                                                                 through the same comparator
 * One line per checked tensor:
 *   CHECK <case> <tensor> elems=<n> mismatches=<m> first=<index> ref=<hex> got=<hex>
 * (HASH <case> <tensor> elems=<n> fnv1a=<hex> with --ref-only alone); exit status 0 only if every
 * m is 0 and every refusal behaved.
 *
 * "Model" tensors (Q4_0 weights, F32 caches) live in a second context outside the eval arena, as
 * the reference's model does (vsim.cpp:253-265).  Every compute gets its work buffer before the
 * snapshot, so ggml_graph_compute allocates nothing and the arena's object list stays as it was. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ggml.h"
#include "../include/vsim_hip.h"

enum { MODE_DEVICE, MODE_REF_ONLY, MODE_REF_VS_REF };

#define ARENA_BYTES ((size_t)8 << 20)
#define MODEL_BYTES ((size_t)4 << 20)
#define SLAB_BYTES ((size_t)64 << 10)
#define WORK_BYTES ((size_t)512 << 10)

typedef struct {
  struct ggml_context *ctx;
  char *buf;
} Arena;

typedef struct {
  const char *name;
  struct ggml_tensor *t;
} Check;

static int g_mode = MODE_DEVICE, g_T = 1, g_U = 1, g_bad = 0;
static const char *g_case = "";
static Arena A, B;                 /* eval arenas */
static struct ggml_context *MC;    /* model context */
static char *g_model, *g_slab;     /* its buffer; a slab for leafs at a fixed address */
static char *g_snap[4];
static struct ggml_cgraph G[4];

static char *region(int i) { return i == 0 ? A.buf : i == 1 ? B.buf : i == 2 ? g_model : g_slab; }
static size_t region_bytes(int i) { return i < 2 ? ARENA_BYTES : i == 2 ? MODEL_BYTES : SLAB_BYTES; }
static void snapshot(void) { for (int i = 0; i < 4; ++i) memcpy(g_snap[i], region(i), region_bytes(i)); }
static void restore(void) { for (int i = 0; i < 4; ++i) memcpy(region(i), g_snap[i], region_bytes(i)); }
static int untouched(void) {
  for (int i = 0; i < 4; ++i) if (memcmp(g_snap[i], region(i), region_bytes(i))) return 0;
  return 1;
}

/* ------------------------------------------------------------------ fills */
static uint32_t g_lcg = 1;
static uint32_t lcg(void) { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }
static float lcgf(void) { return (float)((int)(lcg() & 0xffff) - 32768) / 16384.0f; } /* [-2, 2) */

static int nel(const struct ggml_tensor *t) { return t->ne[0] * t->ne[1] * t->ne[2] * t->ne[3]; }
static struct ggml_tensor *fill(struct ggml_tensor *t) {
  if (t->type == GGML_TYPE_Q4_0) { /* 20-byte blocks: fp32 scale, 32 nibbles */
    const size_t nb = ggml_nbytes(t) / 20;
    for (size_t b = 0; b < nb; ++b) {
      char *p = (char *)t->data + b * 20;
      const float d = (float)(1 + lcg() % 24) / 512.0f * ((lcg() & 1) ? -1.0f : 1.0f);
      memcpy(p, &d, 4);
      for (int i = 0; i < 16; ++i) p[4 + i] = (char)(lcg() & 0xff);
    }
  } else {
    float *p = (float *)t->data;
    for (int i = 0; i < nel(t); ++i) p[i] = lcgf();
  }
  return t;
}
static struct ggml_tensor *newt(struct ggml_context *c, enum ggml_type ty, int nd, int n0, int n1, int n2, int n3) {
  const int ne[4] = {n0, n1, n2, n3};
  return ggml_new_tensor(c, ty, nd, ne);
}
/* a filled F32 leaf in context c */
static struct ggml_tensor *leaf(struct ggml_context *c, int nd, int n0, int n1, int n2, int n3) {
  return fill(newt(c, GGML_TYPE_F32, nd, n0, n1, n2, n3));
}
static struct ggml_tensor *q4(int K, int M) { return fill(ggml_new_tensor_2d(MC, GGML_TYPE_Q4_0, K, M)); }
static struct ggml_tensor *ids(struct ggml_context *c, const int *v, int n) {
  struct ggml_tensor *t = ggml_new_tensor_1d(c, GGML_TYPE_I32, n);
  memcpy(t->data, v, (size_t)n * 4);
  return t;
}
static struct ggml_cgraph *graph(int i) {
  memset(&G[i], 0, sizeof G[i]);
  return &G[i];
}

/* ------------------------------------------------------------------ comparator */
static uint32_t *elements(const struct ggml_tensor *t) { /* logical order, by ne / nb */
  uint32_t *out = malloc((size_t)nel(t) * 4 + 4), *o = out;
  for (int i3 = 0; i3 < t->ne[3]; ++i3)
    for (int i2 = 0; i2 < t->ne[2]; ++i2)
      for (int i1 = 0; i1 < t->ne[1]; ++i1)
        for (int i0 = 0; i0 < t->ne[0]; ++i0)
          memcpy(o++, (const char *)t->data + i0 * t->nb[0] + i1 * t->nb[1] + i2 * t->nb[2] + i3 * t->nb[3], 4);
  return out;
}
static void compare(const char *name, int n, const uint32_t *ref, const uint32_t *got) {
  int m = 0, first = -1;
  for (int i = 0; i < n; ++i)
    if (ref[i] != got[i] && m++ == 0) first = i;
  printf("CHECK %s %s elems=%d mismatches=%d first=%d ref=%08x got=%08x\n", g_case, name, n, m, first,
         first < 0 ? 0u : ref[first], first < 0 ? 0u : got[first]);
  if (m) g_bad = 1;
}
static void hash(const char *name, int n, const uint32_t *v) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < n; ++i)
    for (int b = 0; b < 4; ++b) h = (h ^ ((v[i] >> (8 * b)) & 0xff)) * 1099511628211ull;
  printf("HASH %s %s elems=%d fnv1a=%016llx\n", g_case, name, n, (unsigned long long)h);
}
static void give_work(Arena *a, struct ggml_cgraph *g) {
  if (g->work) return;
  g->work = ggml_new_tensor_1d(a->ctx, GGML_TYPE_I8, WORK_BYTES);
  g->work_size = WORK_BYTES;
}
static void ref_compute(Arena *a, struct ggml_cgraph *g, int threads) {
  g->n_threads = threads; /* <= 0: the reference takes 8 (ggml.c:8246) and writes that back */
  ggml_graph_compute(a->ctx, g);
}

/* One compute of g, reference first, then the device (or the reference at g_U threads) from the
 * same snapshot.  Checked tensors: logical elements; a contiguous external tensor is thereby
 * checked whole.  may_refuse: VSIM_EINVAL with memory untouched also passes.
 * Returns 1 if the device refused. */
static int run_opt(Arena *a, struct ggml_cgraph *g, const Check *c, int n, int may_refuse) {
  uint32_t *ref[16];
  give_work(a, g);
  snapshot();
  ref_compute(a, g, g_T);
  for (int i = 0; i < n; ++i) ref[i] = elements(c[i].t);
  if (g_mode == MODE_REF_ONLY) {
    for (int i = 0; i < n; ++i) { hash(c[i].name, nel(c[i].t), ref[i]); free(ref[i]); }
    return 0;
  }
  restore();
  if (g_mode == MODE_REF_VS_REF) {
    ref_compute(a, g, g_U);
  } else {
    g->n_threads = g_T;
    const int rc = vsim_graph_compute_rc(a->ctx, g);
    if (rc == VSIM_EINVAL && may_refuse) {
      const int same = untouched();
      printf("REFUSED %s untouched=%d error=\"%s\"\n", g_case, same, vsim_last_error());
      if (!same) g_bad = 1;
      for (int i = 0; i < n; ++i) free(ref[i]);
      return 1;
    }
    if (rc != VSIM_OK) {
      printf("ERROR %s vsim_graph_compute_rc=%d: %s\n", g_case, rc, vsim_last_error());
      exit(1);
    }
    for (int i = 0; i < n; ++i)
      if (vsim_graph_sync_tensor(c[i].t) != VSIM_OK) {
        printf("ERROR %s vsim_graph_sync_tensor(%s): %s\n", g_case, c[i].name, vsim_last_error());
        exit(1);
      }
  }
  for (int i = 0; i < n; ++i) {
    uint32_t *got = elements(c[i].t);
    compare(c[i].name, nel(c[i].t), ref[i], got);
    free(got);
    free(ref[i]);
  }
  return 0;
}
static void run(Arena *a, struct ggml_cgraph *g, const Check *c, int n) { (void)run_opt(a, g, c, n, 0); }
static void run1(Arena *a, struct ggml_tensor *out, const char *name) {
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, out);
  const Check c[1] = {{name, out}};
  run(a, g, c, 1);
}

/* A graph the device must refuse in its dry pass: VSIM_EINVAL naming the op, arena and externals
 * byte-identical, the computes counter unchanged.  The reference is not run (it asserts on some). */
static void refuse(Arena *a, struct ggml_cgraph *g, int op) {
  if (g_mode != MODE_DEVICE) {
    printf("SKIP %s refusal (reference not run on it)\n", g_case);
    return;
  }
  char want[32];
  uint64_t c0 = 0, c1 = 0;
  give_work(a, g);
  snapshot();
  vsim_graph_stats(&c0, NULL, NULL, NULL);
  g->n_threads = g_T;
  const int rc = vsim_graph_compute_rc(a->ctx, g);
  const char *err = vsim_last_error();
  vsim_graph_stats(&c1, NULL, NULL, NULL);
  snprintf(want, sizeof want, "(op %d,", op);
  const int named = rc == VSIM_EINVAL && err && strstr(err, want) != NULL, same = untouched();
  printf("REFUSE %s rc=%d named=%d untouched=%d computes_same=%d error=\"%s\"\n", g_case, rc, named, same,
         (int)(c0 == c1), err ? err : "");
  if (rc != VSIM_EINVAL || !named || !same || c0 != c1) g_bad = 1;
}

/* ------------------------------------------------------------------ dup / cpy */
static void dup_perm(int n0, int n1, int n2, int n3, int a0, int a1, int a2, int a3, int use_cpy) {
  struct ggml_tensor *x = leaf(A.ctx, 4, n0, n1, n2, n3), *p = ggml_permute(A.ctx, x, a0, a1, a2, a3);
  struct ggml_tensor *y = use_cpy ? ggml_cpy(A.ctx, p, newt(A.ctx, GGML_TYPE_F32, 4, p->ne[0], p->ne[1], p->ne[2], p->ne[3]))
                                  : ggml_dup(A.ctx, p);
  run1(&A, y, "out");
}
static void c_dup_perm_0213(void) { dup_perm(7, 5, 3, 2, 0, 2, 1, 3, 0); }
static void c_cpy_perm_1023(void) { dup_perm(7, 5, 3, 2, 1, 0, 2, 3, 1); }
static void c_cpy_perm_2013(void) { dup_perm(33, 9, 4, 2, 2, 0, 1, 3, 1); }
static void c_cpy_cache_view(void) {
  struct ggml_tensor *cache = leaf(MC, 1, 10 * 64, 1, 1, 1), *x = leaf(A.ctx, 2, 64, 5, 1, 1);
  struct ggml_tensor *y = ggml_cpy(A.ctx, x, ggml_view_1d(A.ctx, cache, 5 * 64, (size_t)3 * 64 * 4));
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, y);
  const Check c[2] = {{"out", y}, {"cache", cache}};
  run(&A, g, c, 2);
}

/* ------------------------------------------------------------------ add / mul */
static void binop_padded(int mul) {
  struct ggml_tensor *base = leaf(A.ctx, 2, 80, 7, 1, 1), *b = leaf(A.ctx, 2, 40, 7, 1, 1);
  struct ggml_tensor *a = ggml_view_2d(A.ctx, base, 40, 7, (size_t)2 * 40 * 4, 0);
  run1(&A, mul ? ggml_mul(A.ctx, a, b) : ggml_add(A.ctx, a, b), "out");
}
static void c_add_padded_view(void) { binop_padded(0); }
static void c_mul_padded_view(void) { binop_padded(1); }
static void c_add_transposed_src1(void) {
  struct ggml_tensor *a = leaf(A.ctx, 2, 17, 17, 1, 1), *b = leaf(A.ctx, 2, 17, 17, 1, 1);
  run1(&A, ggml_add(A.ctx, a, ggml_transpose(A.ctx, b)), "out");
}
static void c_addmul_3d(void) {
  struct ggml_tensor *a = leaf(A.ctx, 3, 40, 7, 3, 1), *b = leaf(A.ctx, 3, 40, 7, 3, 1), *c3 = leaf(A.ctx, 3, 40, 7, 3, 1);
  struct ggml_tensor *s = ggml_add(A.ctx, a, b), *y = ggml_mul(A.ctx, s, c3);
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, y);
  const Check c[2] = {{"sum", s}, {"out", y}};
  run(&A, g, c, 2);
}

/* ------------------------------------------------------------------ repeat */
static void repeat(int s0, int s1, int d0, int d1) {
  struct ggml_tensor *a = leaf(A.ctx, s1 > 1 || s0 == 1 ? 2 : 1, s0, s1, 1, 1);
  struct ggml_tensor *shape = newt(A.ctx, GGML_TYPE_F32, 2, d0, d1, 1, 1);
  run1(&A, ggml_repeat(A.ctx, a, shape), "out");
}
static void c_repeat_rows(void) { repeat(96, 1, 96, 5); }
static void c_repeat_cols(void) { repeat(1, 6, 24, 6); }
static void c_repeat_both(void) { repeat(8, 2, 24, 6); }

/* ------------------------------------------------------------------ scale */
static void c_scale_leaf(void) {
  struct ggml_tensor *x = leaf(A.ctx, 3, 13, 5, 3, 1);
  run1(&A, ggml_scale(A.ctx, x, ggml_new_f32(A.ctx, 0.3721f)), "out");
}
/* the scalar is itself a node: its value exists only once the graph runs */
static void c_scale_node_scalar(void) {
  struct ggml_tensor *x = leaf(A.ctx, 3, 13, 5, 3, 1);
  struct ggml_tensor *s = ggml_mul(A.ctx, ggml_new_f32(A.ctx, 0.75f), ggml_new_f32(A.ctx, -1.3f));
  struct ggml_tensor *y = ggml_scale(A.ctx, x, s);
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, y);
  const Check c[1] = {{"out", y}};
  if (run_opt(&A, g, c, 1, 1)) { /* refused: a valid graph right after must pass */
    struct ggml_tensor *x2 = leaf(A.ctx, 3, 13, 5, 3, 1);
    run1(&A, ggml_scale(A.ctx, x2, ggml_new_f32(A.ctx, -0.975f)), "after");
  }
}

/* ------------------------------------------------------------------ diag_mask_inf, soft_max */
static void mask(int nc, int nr, int nz, int n_past, int equal, int soft) {
  struct ggml_tensor *x = leaf(A.ctx, 3, nc, nr, nz, 1);
  if (equal)
    for (int i = 0; i < nc; ++i) ((float *)x->data)[nc + i] = 0.25f; /* row 1 (row 0 if nr == 1) */
  struct ggml_tensor *y = ggml_diag_mask_inf(A.ctx, x, n_past);
  run1(&A, soft ? ggml_soft_max(A.ctx, y) : y, "out");
}
static void c_mask_only(void) { mask(13, 5, 3, 8, 0, 0); }
static void c_mask_past8(void) { mask(13, 5, 3, 8, 0, 1); }
static void c_mask_past0(void) { mask(13, 5, 3, 0, 0, 1); }
static void c_mask_one_row(void) { mask(13, 1, 3, 12, 0, 1); }
static void c_mask_one_col(void) { mask(1, 1, 3, 0, 0, 1); }
static void c_mask_300_cols(void) { mask(300, 5, 3, 295, 0, 1); }
static void c_mask_equal_row(void) { mask(13, 5, 3, 8, 1, 1); }

/* ------------------------------------------------------------------ norm, mul, add as the model does */
static void norm(int n, int rows) {
  struct ggml_tensor *x = leaf(A.ctx, 2, n, rows, 1, 1), *w = leaf(MC, 1, n, 1, 1, 1), *b = leaf(MC, 1, n, 1, 1, 1);
  struct ggml_tensor *y = ggml_norm(A.ctx, x);
  struct ggml_tensor *z = ggml_add(A.ctx, ggml_mul(A.ctx, ggml_repeat(A.ctx, w, y), y), ggml_repeat(A.ctx, b, y));
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, z);
  const Check c[2] = {{"norm", y}, {"out", z}};
  run(&A, g, c, 2);
}
static void c_norm_32x1(void) { norm(32, 1); }
static void c_norm_32x5(void) { norm(32, 5); }
static void c_norm_96x1(void) { norm(96, 1); }
static void c_norm_96x5(void) { norm(96, 5); }
static void c_norm_1000x1(void) { norm(1000, 1); }
static void c_norm_1000x5(void) { norm(1000, 5); }

/* ------------------------------------------------------------------ gelu */
static void c_gelu_1000(void) {
  static const float edge[] = {0.0f, -0.0f, 10.0f, -10.0f, 65504.0f, -65504.0f};
  struct ggml_tensor *x = leaf(A.ctx, 1, 1000, 1, 1, 1);
  for (int i = 500; i < 1000; ++i) ((float *)x->data)[i] *= 4.0f;
  for (int i = 0; i < 6; ++i) ((float *)x->data)[i * 157 + 3] = edge[i]; /* 65504: the largest finite fp16 */
  run1(&A, ggml_gelu(A.ctx, x), "out");
}

/* ------------------------------------------------------------------ get_rows */
static void get_rows(int n) {
  static const int id[9] = {0, 49, 7, 7, 0, 31, 48, 1, 49};
  struct ggml_tensor *w = q4(64, 50);
  run1(&A, ggml_get_rows(A.ctx, w, ids(A.ctx, id, n)), "out");
}
static void c_get_rows_1(void) { get_rows(1); }
static void c_get_rows_9(void) { get_rows(9); }

/* ------------------------------------------------------------------ Q4_0 mul_mat */
static void mmq(int M, int K, int N) {
  struct ggml_tensor *w = q4(K, M), *x = leaf(A.ctx, 2, K, N, 1, 1);
  run1(&A, ggml_mul_mat(A.ctx, w, x), "out");
}
static void c_mmq_1_32_1(void) { mmq(1, 32, 1); }
static void c_mmq_33_64_2(void) { mmq(33, 64, 2); }
static void c_mmq_130_96_9(void) { mmq(130, 96, 9); }
static void c_mmq_gather_rows(void) { /* src1 rows (K + 32) floats apart */
  const int M = 33, K = 64, N = 5;
  struct ggml_tensor *base = leaf(A.ctx, 2, K + 32, N, 1, 1);
  struct ggml_tensor *w = q4(K, M);
  run1(&A, ggml_mul_mat(A.ctx, w, ggml_view_2d(A.ctx, base, K, N, (size_t)(K + 32) * 4, 0)), "out");
}
static void c_mmq_small_then_large(void) { /* the scratch rows regrow between two nodes of one graph */
  struct ggml_tensor *w1 = q4(32, 3), *w2 = q4(96, 130), *w3 = q4(160, 70);
  struct ggml_tensor *b1 = leaf(A.ctx, 2, 32, 1, 1, 1), *b2 = leaf(A.ctx, 2, 96 + 32, 9, 1, 1), *b3 = leaf(A.ctx, 2, 160, 21, 1, 1);
  struct ggml_tensor *y1 = ggml_mul_mat(A.ctx, w1, b1);
  struct ggml_tensor *y2 = ggml_mul_mat(A.ctx, w2, ggml_view_2d(A.ctx, b2, 96, 9, (size_t)(96 + 32) * 4, 0));
  struct ggml_tensor *y3 = ggml_mul_mat(A.ctx, w3, b3);
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, y1);
  ggml_build_forward_expand(g, y2);
  ggml_build_forward_expand(g, y3);
  const Check c[3] = {{"small", y1}, {"gathered", y2}, {"large", y3}};
  run(&A, g, c, 3);
}

/* ------------------------------------------------------------------ F32 mul_mat */
/* K and Q as gptneox_eval builds them from the cache view (vsim.cpp:560-585) */
static void c_kq_cache_view(void) {
  const int d = 16, H = 3, N = 5, n_past = 8, nk = n_past + N, E = d * H, n_rot = 8;
  struct ggml_tensor *memk = leaf(MC, 1, 20 * E, 1, 1, 1), *qcur = leaf(A.ctx, 2, E, N, 1, 1);
  struct ggml_tensor *Q = ggml_permute(
      A.ctx, ggml_gptneox_rope(A.ctx, ggml_cpy(A.ctx, qcur, ggml_new_tensor_3d(A.ctx, GGML_TYPE_F32, d, H, N)), n_past, n_rot, 0),
      0, 2, 1, 3);
  struct ggml_tensor *K = ggml_permute(
      A.ctx, ggml_gptneox_rope(A.ctx, ggml_reshape_3d(A.ctx, ggml_view_1d(A.ctx, memk, nk * E, 0), d, H, nk), n_past, n_rot, 1),
      0, 2, 1, 3);
  struct ggml_tensor *KQ = ggml_mul_mat(A.ctx, K, Q);
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, KQ);
  const Check c[2] = {{"kq", KQ}, {"memory_k", memk}};
  run(&A, g, c, 2);
}
static void c_kq_4d(void) {
  struct ggml_tensor *k = leaf(A.ctx, 4, 16, 13, 3, 2), *q = leaf(A.ctx, 4, 16, 5, 3, 2);
  run1(&A, ggml_mul_mat(A.ctx, k, q), "out");
}
/* V_trans from the cache view, KQV and the head merge (vsim.cpp:598-615): the sums are grouped
 * by the thread count */
static void kqv(int nk) {
  const int d = 16, H = 3, N = 5, E = d * H;
  struct ggml_tensor *memv = leaf(MC, 1, 20 * E, 1, 1, 1), *p = leaf(A.ctx, 3, nk, N, H, 1);
  struct ggml_tensor *Vt =
      ggml_permute(A.ctx, ggml_reshape_3d(A.ctx, ggml_view_1d(A.ctx, memv, nk * E, 0), d, H, nk), 1, 2, 0, 3);
  struct ggml_tensor *KQV = ggml_mul_mat(A.ctx, Vt, p);
  struct ggml_tensor *cur = ggml_cpy(A.ctx, ggml_permute(A.ctx, KQV, 0, 2, 1, 3), ggml_new_tensor_2d(A.ctx, GGML_TYPE_F32, E, N));
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, cur);
  const Check c[2] = {{"kqv", KQV}, {"merged", cur}};
  run(&A, g, c, 2);
}
static void c_kqv(void) { kqv(13); }
static void c_kqv_2_keys(void) { kqv(2); }
static void c_kqv_4d(void) { /* src0 [16,13,3,2] transposed in dims 0/1 */
  struct ggml_tensor *v = leaf(A.ctx, 4, 16, 13, 3, 2), *p = leaf(A.ctx, 4, 13, 5, 3, 2);
  run1(&A, ggml_mul_mat(A.ctx, ggml_transpose(A.ctx, v), p), "out");
}

/* ------------------------------------------------------------------ rope */
static struct ggml_tensor *rope(int neox, struct ggml_tensor *x, int n_past, int n_dims, int mode) {
  return neox ? ggml_gptneox_rope(A.ctx, x, n_past, n_dims, mode) : ggml_rope(A.ctx, x, n_past, n_dims, mode);
}
static void rope_case(int neox, int T, int n_past, int n_dims, int mode) {
  run1(&A, rope(neox, leaf(A.ctx, 3, 32, 3, T, 1), n_past, n_dims, mode), "out");
}
static void c_rope_d8_p0(void) { rope_case(0, 5, 0, 8, 0); }
static void c_rope_d8_p3(void) { rope_case(0, 5, 3, 8, 0); }
static void c_rope_d32_p0(void) { rope_case(0, 5, 0, 32, 0); }
static void c_rope_d32_p3(void) { rope_case(0, 5, 3, 32, 0); }
static void c_rope_mode1(void) { rope_case(0, 9, 6, 8, 1); }
static void c_neox_rope_d8_p0(void) { rope_case(1, 5, 0, 8, 0); }
static void c_neox_rope_d8_p3(void) { rope_case(1, 5, 3, 8, 0); }
static void c_neox_rope_d32_p0(void) { rope_case(1, 5, 0, 32, 0); }
static void c_neox_rope_d32_p3(void) { rope_case(1, 5, 3, 32, 0); }
static void c_neox_rope_mode1(void) { rope_case(1, 9, 6, 8, 1); }
static void rope_regrow(int neox) { /* position 600 after a compute at position 3 */
  const int past[2] = {3, 600};
  for (int i = 0; i < 2; ++i) {
    struct ggml_tensor *y = rope(neox, leaf(A.ctx, 3, 32, 3, 5, 1), past[i], 8, 0);
    struct ggml_cgraph *g = graph(i);
    ggml_build_forward_expand(g, y);
    const Check c[1] = {{i ? "past600" : "past3", y}};
    run(&A, g, c, 1);
  }
}
static void c_rope_regrow(void) { rope_regrow(0); }
static void c_neox_rope_regrow(void) { rope_regrow(1); }
static void c_rope_two_dims(void) { /* one graph, n_dims 8, 32, 32, 8 */
  struct ggml_tensor *x = leaf(A.ctx, 3, 32, 3, 5, 1);
  run1(&A, rope(1, rope(1, rope(0, rope(0, x, 2, 8, 0), 1, 32, 0), 4, 32, 0), 0, 8, 0), "out");
}

/* ------------------------------------------------------------------ mirror lifecycle */
static struct ggml_tensor *small_net(Arena *a, struct ggml_tensor *w, struct ggml_tensor *bias, int N) {
  struct ggml_tensor *y = ggml_mul_mat(a->ctx, w, leaf(a->ctx, 2, w->ne[0], N, 1, 1));
  return ggml_add(a->ctx, y, ggml_repeat(a->ctx, bias, y));
}
static void c_life_two_arenas(void) { /* arena A, arena B (another buffer), arena A again */
  struct ggml_tensor *w = q4(64, 33), *bias = leaf(MC, 1, 33, 1, 1, 1);
  Arena *seq[3] = {&A, &B, &A};
  const char *name[3] = {"a1", "b", "a2"};
  for (int i = 0; i < 3; ++i) {
    struct ggml_tensor *y = small_net(seq[i], w, bias, 2 + i);
    struct ggml_cgraph *g = graph(i);
    ggml_build_forward_expand(g, y);
    const Check c[1] = {{name[i], y}};
    run(seq[i], g, c, 1);
  }
}
/* an external F32 leaf freed and re-created at the same address with another ne[1] */
static void c_life_leaf_reshaped(void) {
  const int rows[2] = {4, 9};
  for (int i = 0; i < 2; ++i) {
    struct ggml_tensor *e = ggml_new_tensor_2d(MC, GGML_TYPE_F32, 16, rows[i]);
    e->data = g_slab;
    fill(e);
    struct ggml_tensor *y = ggml_add(A.ctx, leaf(A.ctx, 2, 16, rows[i], 1, 1), e);
    struct ggml_cgraph *g = graph(i);
    ggml_build_forward_expand(g, y);
    const Check c[1] = {{i ? "rows9" : "rows4", y}};
    run(&A, g, c, 1);
  }
}
/* vsim_graph_reset, then the same leaf with new contents: they must be seen */
static void c_life_reset(void) {
  struct ggml_tensor *e = leaf(MC, 2, 16, 4, 1, 1), *w = q4(64, 33), *bias = leaf(MC, 1, 33, 1, 1, 1);
  for (int i = 0; i < 2; ++i) {
    if (i) {
      if (g_mode == MODE_DEVICE) vsim_graph_reset();
      fill(e);
      fill(w);
    }
    struct ggml_tensor *y = ggml_add(A.ctx, leaf(A.ctx, 2, 16, 4, 1, 1), e), *z = small_net(&A, w, bias, 3);
    struct ggml_cgraph *g = graph(i);
    ggml_build_forward_expand(g, y);
    ggml_build_forward_expand(g, z);
    const Check c[2] = {{i ? "after.f32" : "before.f32", y}, {i ? "after.q4" : "before.q4", z}};
    run(&A, g, c, 2);
  }
}
/* vsim_graph_sync_tensor on a strided view: host bytes outside the view's span stay as they were */
static void c_life_sync_view(void) {
  struct ggml_tensor *a = leaf(A.ctx, 2, 40, 7, 1, 1), *b = leaf(A.ctx, 2, 40, 7, 1, 1);
  struct ggml_tensor *y = ggml_add(A.ctx, a, b);
  struct ggml_tensor *v = ggml_view_2d(A.ctx, y, 10, 3, (size_t)40 * 4, (size_t)(40 * 2 + 4) * 4);
  struct ggml_cgraph *g = graph(0);
  ggml_build_forward_expand(g, v);
  const Check c[1] = {{"view", v}};
  run(&A, g, c, 1);
  if (g_mode != MODE_DEVICE) return;
  /* host now holds the device's view bytes; poison the whole node, sync the view alone */
  uint32_t *want = elements(v);
  const size_t total = (size_t)40 * 7 * 4, lo = (size_t)(40 * 2 + 4) * 4, hi = lo + (size_t)(2 * 40 + 10) * 4;
  memset(y->data, 0xa5, total);
  if (vsim_graph_sync_tensor(v) != VSIM_OK) { printf("ERROR %s sync: %s\n", g_case, vsim_last_error()); exit(1); }
  uint32_t *got = elements(v);
  compare("view.resynced", nel(v), want, got);
  int outside = 0;
  for (size_t i = 0; i < total; ++i)
    if ((i < lo || i >= hi) && ((unsigned char *)y->data)[i] != 0xa5) ++outside;
  printf("CHECK %s bytes.outside.span elems=%d mismatches=%d first=-1 ref=00000000 got=00000000\n", g_case,
         (int)(total - (hi - lo)), outside);
  if (outside) g_bad = 1;
  free(want);
  free(got);
}

/* ------------------------------------------------------------------ refusals */
/* the refused node sits between valid ones; a valid graph right after must pass */
static void refusal(int kind) {
  struct ggml_context *c = A.ctx;
  struct ggml_tensor *x0 = leaf(c, 3, 13, 5, 3, 1), *x1 = leaf(c, 3, 13, 5, 3, 1);
  struct ggml_tensor *x = ggml_add(c, x0, x1), *bad = NULL, *end = NULL;
  struct ggml_cgraph *g = graph(0);
  int op = 0;
  if (kind == 0) {
    bad = ggml_alibi(c, x, 2, 3);
    op = GGML_OP_ALIBI;
  } else if (kind == 1) {
    bad = ggml_silu(c, x);
    op = GGML_OP_SILU;
  } else if (kind == 2) { /* destination: a permuted tensor */
    bad = ggml_cpy(c, x, ggml_permute(c, newt(c, GGML_TYPE_F32, 3, 5, 13, 3, 1), 1, 0, 2, 3));
    op = GGML_OP_CPY;
  } else if (kind == 3) {
    bad = ggml_cpy(c, x, newt(c, GGML_TYPE_F16, 3, 13, 5, 3, 1));
    op = GGML_OP_CPY;
  } else {
    static const int id[3] = {4, 0, 49};
    bad = ggml_get_rows(c, leaf(MC, 2, 64, 50, 1, 1), ids(c, id, 3));
    op = GGML_OP_GET_ROWS;
  }
  ggml_build_forward_expand(g, bad);
  if (kind == 0 || kind == 1) {
    end = ggml_add(c, bad, leaf(c, 3, 13, 5, 3, 1));
  } else {
    end = ggml_mul(c, x, leaf(c, 3, 13, 5, 3, 1));
  }
  ggml_build_forward_expand(g, end);
  refuse(&A, g, op);
  struct ggml_tensor *w = q4(64, 33), *bias = leaf(MC, 1, 33, 1, 1, 1);
  struct ggml_tensor *y = small_net(&A, w, bias, 4);
  struct ggml_cgraph *g2 = graph(1);
  ggml_build_forward_expand(g2, y);
  const Check ck[1] = {{"after", y}};
  run(&A, g2, ck, 1);
}
static void c_refuse_alibi(void) { refusal(0); }
static void c_refuse_silu(void) { refusal(1); }
static void c_refuse_cpy_strided_dst(void) { refusal(2); }
static void c_refuse_cpy_f16(void) { refusal(3); }
static void c_refuse_get_rows_f32(void) { refusal(4); }

/* ------------------------------------------------------------------ composite: two GPT-J-style layers */
/* gptneox_eval's node sequence (vsim.cpp:514-724, parallel residual) with ggml_rope for
 * gptneox_rope and no attention biases; a 5-token batch at n_past 0, then one token on top,
 * which must stay on the per-node path. */
enum { CE = 64, CH = 4, CD = 16, CROT = 8, CV = 96, CL = 2, CCTX = 16 };
typedef struct {
  struct ggml_tensor *ln1w, *ln1b, *ln2w, *ln2b, *wq, *wk, *wv, *wo, *wfc, *bfc, *wproj, *bproj;
} CLayer;
static struct ggml_tensor *affine(struct ggml_context *c, struct ggml_tensor *x, struct ggml_tensor *w, struct ggml_tensor *b) {
  struct ggml_tensor *cur = ggml_norm(c, x);
  return ggml_add(c, ggml_mul(c, ggml_repeat(c, w, cur), cur), ggml_repeat(c, b, cur));
}
static void c_gptj_two_layers(void) {
  struct ggml_context *c = A.ctx;
  CLayer Y[CL];
  struct ggml_tensor *wte = q4(CE, CV), *lmh = q4(CE, CV), *lnfw = leaf(MC, 1, CE, 1, 1, 1), *lnfb = leaf(MC, 1, CE, 1, 1, 1);
  struct ggml_tensor *memk = leaf(MC, 1, CL * CCTX * CE, 1, 1, 1), *memv = leaf(MC, 1, CL * CCTX * CE, 1, 1, 1);
  for (int il = 0; il < CL; ++il) {
    CLayer *y = &Y[il]; /* one fill per statement: the order is part of the case */
    y->ln1w = leaf(MC, 1, CE, 1, 1, 1);
    y->ln1b = leaf(MC, 1, CE, 1, 1, 1);
    y->ln2w = leaf(MC, 1, CE, 1, 1, 1);
    y->ln2b = leaf(MC, 1, CE, 1, 1, 1);
    y->wq = q4(CE, CE);
    y->wk = q4(CE, CE);
    y->wv = q4(CE, CE);
    y->wo = q4(CE, CE);
    y->wfc = q4(CE, 4 * CE);
    y->bfc = leaf(MC, 1, 4 * CE, 1, 1, 1);
    y->wproj = q4(4 * CE, CE);
    y->bproj = leaf(MC, 1, CE, 1, 1, 1);
  }
  static const int tok[6] = {5, 95, 0, 41, 41, 17};
  for (int step = 0; step < 2; ++step) {
    const int N = step ? 1 : 5, n_past = step ? 5 : 0;
    struct ggml_cgraph *g = graph(step);
    struct ggml_tensor *inpL = ggml_get_rows(c, wte, ids(c, tok + n_past, N));
    for (int il = 0; il < CL; ++il) {
      const size_t row = (size_t)4 * CE;
      struct ggml_tensor *cur = affine(c, inpL, Y[il].ln1w, Y[il].ln1b);
      struct ggml_tensor *Qcur = ggml_mul_mat(c, Y[il].wq, cur), *Kcur = ggml_mul_mat(c, Y[il].wk, cur);
      struct ggml_tensor *Vcur = ggml_mul_mat(c, Y[il].wv, cur);
      ggml_build_forward_expand(g, ggml_cpy(c, Kcur, ggml_view_1d(c, memk, N * CE, row * (il * CCTX + n_past))));
      ggml_build_forward_expand(g, ggml_cpy(c, Vcur, ggml_view_1d(c, memv, N * CE, row * (il * CCTX + n_past))));
      struct ggml_tensor *Q = ggml_permute(
          c, ggml_rope(c, ggml_cpy(c, Qcur, ggml_new_tensor_3d(c, GGML_TYPE_F32, CD, CH, N)), n_past, CROT, 0), 0, 2, 1, 3);
      struct ggml_tensor *K = ggml_permute(
          c, ggml_rope(c, ggml_reshape_3d(c, ggml_view_1d(c, memk, (n_past + N) * CE, row * il * CCTX), CD, CH, n_past + N),
                       n_past, CROT, 1),
          0, 2, 1, 3);
      struct ggml_tensor *KQ = ggml_soft_max(
          c, ggml_diag_mask_inf(c, ggml_scale(c, ggml_mul_mat(c, K, Q), ggml_new_f32(c, 1.0f / sqrtf((float)CD))), n_past));
      struct ggml_tensor *Vt = ggml_permute(
          c, ggml_reshape_3d(c, ggml_view_1d(c, memv, (n_past + N) * CE, row * il * CCTX), CD, CH, n_past + N), 1, 2, 0, 3);
      struct ggml_tensor *KQV = ggml_mul_mat(c, Vt, KQ);
      cur = ggml_cpy(c, ggml_permute(c, KQV, 0, 2, 1, 3), ggml_new_tensor_2d(c, GGML_TYPE_F32, CE, N));
      cur = ggml_mul_mat(c, Y[il].wo, cur);
      struct ggml_tensor *ff = affine(c, inpL, Y[il].ln2w, Y[il].ln2b);
      ff = ggml_mul_mat(c, Y[il].wfc, ff);
      ff = ggml_gelu(c, ggml_add(c, ggml_repeat(c, Y[il].bfc, ff), ff));
      ff = ggml_mul_mat(c, Y[il].wproj, ff);
      ff = ggml_add(c, ggml_repeat(c, Y[il].bproj, ff), ff);
      inpL = ggml_add(c, inpL, ggml_add(c, cur, ff));
    }
    inpL = ggml_mul_mat(c, lmh, affine(c, inpL, lnfw, lnfb));
    ggml_build_forward_expand(g, inpL);
    const Check ck[3] = {{step ? "token.logits" : "batch.logits", inpL},
                         {step ? "token.memory_k" : "batch.memory_k", memk},
                         {step ? "token.memory_v" : "batch.memory_v", memv}};
    run(&A, g, ck, 3);
  }
  if (g_mode == MODE_DEVICE) {
    uint64_t fast = 0, plans = 0;
    vsim_graph_fast_stats(&fast, &plans);
    printf("FASTPATH %s fast_evals=%llu plans=%llu\n", g_case, (unsigned long long)fast, (unsigned long long)plans);
    if (fast || plans) g_bad = 1;
  }
}

/* ------------------------------------------------------------------ table, main */
#define CASE(n) {#n, c_##n}
static const struct { const char *name; void (*fn)(void); } CASES[] = {
    CASE(dup_perm_0213), CASE(cpy_perm_1023), CASE(cpy_perm_2013), CASE(cpy_cache_view),
    CASE(add_padded_view), CASE(mul_padded_view), CASE(add_transposed_src1), CASE(addmul_3d),
    CASE(repeat_rows), CASE(repeat_cols), CASE(repeat_both),
    CASE(scale_leaf), CASE(scale_node_scalar),
    CASE(mask_only), CASE(mask_past8), CASE(mask_past0), CASE(mask_one_row), CASE(mask_one_col),
    CASE(mask_300_cols), CASE(mask_equal_row),
    CASE(norm_32x1), CASE(norm_32x5), CASE(norm_96x1), CASE(norm_96x5), CASE(norm_1000x1), CASE(norm_1000x5),
    CASE(gelu_1000), CASE(get_rows_1), CASE(get_rows_9),
    CASE(mmq_1_32_1), CASE(mmq_33_64_2), CASE(mmq_130_96_9), CASE(mmq_gather_rows), CASE(mmq_small_then_large),
    CASE(kq_cache_view), CASE(kq_4d), CASE(kqv), CASE(kqv_2_keys), CASE(kqv_4d),
    CASE(rope_d8_p0), CASE(rope_d8_p3), CASE(rope_d32_p0), CASE(rope_d32_p3), CASE(rope_mode1),
    CASE(neox_rope_d8_p0), CASE(neox_rope_d8_p3), CASE(neox_rope_d32_p0), CASE(neox_rope_d32_p3),
    CASE(neox_rope_mode1), CASE(rope_regrow), CASE(neox_rope_regrow), CASE(rope_two_dims),
    CASE(life_two_arenas), CASE(life_leaf_reshaped), CASE(life_reset), CASE(life_sync_view),
    CASE(refuse_alibi), CASE(refuse_silu), CASE(refuse_cpy_strided_dst), CASE(refuse_cpy_f16),
    CASE(refuse_get_rows_f32),
    CASE(gptj_two_layers),
};
#define NCASES ((int)(sizeof CASES / sizeof CASES[0]))

static struct ggml_context *ctx_on(char *buf, size_t bytes) {
  struct ggml_init_params ip = {.mem_size = bytes, .mem_buffer = buf};
  return ggml_init(ip);
}

int main(int argc, char **argv) {
  int against = 0, ref_only = 0, which = -1;
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (int i = 0; i < NCASES; ++i) puts(CASES[i].name);
    return 0;
  }
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--threads") && i + 1 < argc) g_T = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--against-threads") && i + 1 < argc) { g_U = atoi(argv[++i]); against = 1; }
    else if (!strcmp(argv[i], "--ref-only")) ref_only = 1;
    else if (which < 0 && argv[i][0] != '-') {
      for (int k = 0; k < NCASES; ++k) if (!strcmp(argv[i], CASES[k].name)) which = k;
      if (which < 0) { fprintf(stderr, "graph_cases: no case %s\n", argv[i]); return 2; }
    } else { fprintf(stderr, "graph_cases: bad argument %s\n", argv[i]); return 2; }
  }
  if (which < 0 || (against && !ref_only)) {
    fprintf(stderr, "usage: graph_cases --list | NAME --threads T [--ref-only [--against-threads U]]\n");
    return 2;
  }
  g_mode = against ? MODE_REF_VS_REF : ref_only ? MODE_REF_ONLY : MODE_DEVICE;
  g_case = CASES[which].name;
  for (const char *p = g_case; *p; ++p) g_lcg = g_lcg * 31u + (unsigned char)*p; /* a seed per case */
  A.buf = malloc(ARENA_BYTES);
  B.buf = malloc(ARENA_BYTES);
  g_model = malloc(MODEL_BYTES);
  g_slab = malloc(SLAB_BYTES);
  for (int i = 0; i < 4; ++i) {
    memset(region(i), 0, region_bytes(i));
    g_snap[i] = malloc(region_bytes(i));
  }
  A.ctx = ctx_on(A.buf, ARENA_BYTES);
  B.ctx = ctx_on(B.buf, ARENA_BYTES);
  MC = ctx_on(g_model, MODEL_BYTES);
  if (!A.ctx || !B.ctx || !MC) { fprintf(stderr, "graph_cases: ggml_init failed\n"); return 2; }
  CASES[which].fn();
  fflush(stdout);
  return g_bad ? 1 : 0;
}
