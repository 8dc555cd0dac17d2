/*
 * batch_check -- batched GPU scans vs stock libyara, buffer by buffer.
 *
 * Test infrastructure: compiles a rule file with the stock libyara compiler,
 * cuts a data file into pieces at the given offsets and scans the list twice
 * with one YR_SCANNER each --
 *   stock:  yr_scanner_scan_mem on every piece in order      (scanner.c:633)
 *   gpu:    yr_gpu_scanner_scan_mem_batch on the whole list   (yr_gpu_scanner.c)
 * -- and compares, piece by piece, the matches ({string idx, offset, length,
 * xor key} of every match of every string, in the scanner's list order), the
 * RULE_MATCHING / RULE_NOT_MATCHING reports and the order of every callback
 * message, plus the return code and the number of pieces finished.  Prints
 * one JSON line; exit status 0 iff everything is equal.
 *
 *   batch_check <rules.yar> <data file> <cuts file>
 *   cuts file: ascending offsets into the data, one per line; the pieces are
 *   [0, c0), [c0, c1), ..., [c_last, size).
 *   BATCH_ARENA=bytes: yr_gpu_scanner_set_batch_arena (several arenas).
 *   BATCH_PREVERIFY=0: pre-verification off (the per-buffer fallback).
 *   BATCH_ERROR_AT=k: the callback returns CALLBACK_ERROR on piece k's first
 *   rule report; both sides must stop there with ERROR_CALLBACK_ERROR.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <yara.h>

#include "yr_gpu_scanner.h"

typedef struct
{
  uint64_t off;
  uint32_t piece, s, len, xk; /* no implicit padding: compared with memcmp */
} match_rec;

typedef struct
{
  uint32_t piece, msg, rule;
} event_rec;

typedef struct
{
  YR_RULES* rules;
  match_rec* m;
  size_t n_m, cap_m;
  event_rec* e;
  size_t n_e, cap_e;
  uint32_t piece;  /* the piece being scanned: SCAN_FINISHED messages seen */
  int dumped;      /* this piece's matches are recorded */
  long error_at;   /* BATCH_ERROR_AT, or -1 */
} collect;

static void push_match(collect* c, match_rec x)
{
  if (c->n_m == c->cap_m)
  {
    c->cap_m = c->cap_m ? 2 * c->cap_m : 1024;
    c->m = (match_rec*) realloc(c->m, c->cap_m * sizeof(match_rec));
  }
  c->m[c->n_m++] = x;
}

static void push_event(collect* c, event_rec x)
{
  if (c->n_e == c->cap_e)
  {
    c->cap_e = c->cap_e ? 2 * c->cap_e : 4096;
    c->e = (event_rec*) realloc(c->e, c->cap_e * sizeof(event_rec));
  }
  c->e[c->n_e++] = x;
}

static int cb(YR_SCAN_CONTEXT* ctx, int msg, void* data, void* user)
{
  collect* c = (collect*) user;
  const int rule_msg = msg == CALLBACK_MSG_RULE_MATCHING || msg == CALLBACK_MSG_RULE_NOT_MATCHING;
  event_rec e = {c->piece, (uint32_t) msg,
                 rule_msg ? (uint32_t) ((YR_RULE*) data - c->rules->rules_table) : 0};
  push_event(c, e);
  if (rule_msg && !c->dumped)
  {
    /* every string's match list as the scan left it */
    for (uint32_t k = 0; k < c->rules->num_strings; k++)
      for (YR_MATCH* m = ctx->matches[k].head; m != NULL; m = m->next)
      {
        match_rec x = {(uint64_t) (m->base + m->offset), c->piece, k, (uint32_t) m->match_length,
                       m->xor_key};
        push_match(c, x);
      }
    c->dumped = 1;
    if (c->error_at >= 0 && (long) c->piece == c->error_at) return CALLBACK_ERROR;
  }
  if (msg == CALLBACK_MSG_SCAN_FINISHED)
  {
    c->piece++;
    c->dumped = 0;
  }
  return CALLBACK_CONTINUE;
}

static uint8_t* load(const char* path, size_t* n)
{
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* b = (uint8_t*) malloc(sz ? sz : 1);
  if (fread(b, 1, sz, f) != (size_t) sz) return NULL;
  fclose(f);
  *n = (size_t) sz;
  return b;
}

static int make_scanner(YR_RULES* rules, collect* c, YR_SCANNER** sc)
{
  int r = yr_scanner_create(rules, sc);
  if (r) return r;
  yr_scanner_set_flags(*sc, SCAN_FLAGS_REPORT_RULES_MATCHING | SCAN_FLAGS_REPORT_RULES_NOT_MATCHING);
  yr_scanner_set_callback(*sc, cb, c);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 4)
  {
    fprintf(stderr, "usage: batch_check rules data cuts\n");
    return 2;
  }
  yr_initialize();
  YR_COMPILER* comp;
  YR_RULES* rules;
  FILE* f = fopen(argv[1], "r");
  if (!f || yr_compiler_create(&comp) || yr_compiler_add_file(comp, f, NULL, argv[1]) ||
      yr_compiler_get_rules(comp, &rules))
  {
    fprintf(stderr, "rule compilation failed\n");
    return 2;
  }
  size_t size = 0;
  uint8_t* data = load(argv[2], &size);
  if (!data)
  {
    fprintf(stderr, "cannot load data\n");
    return 2;
  }
  /* the pieces */
  FILE* cf = fopen(argv[3], "r");
  if (!cf) return 2;
  size_t n = 0, cap = 64;
  const uint8_t** bufs = (const uint8_t**) malloc(cap * sizeof(*bufs));
  size_t* sizes = (size_t*) malloc(cap * sizeof(*sizes));
  size_t at = 0;
  for (;;)
  {
    unsigned long long c;
    const int more = fscanf(cf, "%llu", &c) == 1;
    const size_t end = more ? (size_t) c : size;
    if (end < at || end > size)
    {
      fprintf(stderr, "cuts must ascend within the data\n");
      return 2;
    }
    if (n == cap)
    {
      cap *= 2;
      bufs = (const uint8_t**) realloc(bufs, cap * sizeof(*bufs));
      sizes = (size_t*) realloc(sizes, cap * sizeof(*sizes));
    }
    bufs[n] = data + at;
    sizes[n++] = end - at;
    at = end;
    if (!more) break;
  }
  fclose(cf);

  const long error_at = getenv("BATCH_ERROR_AT") ? atol(getenv("BATCH_ERROR_AT")) : -1;
  collect a = {rules}, b = {rules};
  a.error_at = b.error_at = error_at;

  /* stock: the loop the batch call stands for */
  YR_SCANNER* sc;
  if (make_scanner(rules, &a, &sc)) return 3;
  int rs = ERROR_SUCCESS;
  size_t done_s = 0;
  for (size_t k = 0; k < n; k++)
  {
    rs = yr_scanner_scan_mem(sc, bufs[k], sizes[k]);
    if (rs != ERROR_SUCCESS) break;
    done_s++;
  }
  yr_scanner_destroy(sc);

  /* gpu: one call */
  YR_GPU_RULES* gr;
  YR_GPU_SCANNER* gs;
  int r = yr_gpu_rules_create(rules, 0, &gr);
  if (r == 0) r = yr_gpu_scanner_create(gr, &gs);
  if (r)
  {
    fprintf(stderr, "gpu setup failed: %d\n", r);
    return 3;
  }
  if (getenv("BATCH_ARENA")) yr_gpu_scanner_set_batch_arena(gs, strtoull(getenv("BATCH_ARENA"), NULL, 10));
  const char* pv = getenv("BATCH_PREVERIFY");
  if (pv != NULL && strcmp(pv, "0") == 0) yr_gpu_scanner_set_preverify(gs, 0);
  if (make_scanner(rules, &b, &sc)) return 3;
  size_t done_g = 0;
  const int rg = yr_gpu_scanner_scan_mem_batch(sc, gs, bufs, sizes, n, &done_g);
  yr_scanner_destroy(sc);

  const int same_matches =
      a.n_m == b.n_m && (a.n_m == 0 || memcmp(a.m, b.m, a.n_m * sizeof(match_rec)) == 0);
  const int same_events =
      a.n_e == b.n_e && (a.n_e == 0 || memcmp(a.e, b.e, a.n_e * sizeof(event_rec)) == 0);
  size_t rules_matching = 0;
  for (size_t k = 0; k < a.n_e; k++) rules_matching += a.e[k].msg == CALLBACK_MSG_RULE_MATCHING;
  printf("{\"pieces\": %zu, \"rc_stock\": %d, \"rc_gpu\": %d, \"done_stock\": %zu, "
         "\"done_gpu\": %zu, \"matches_stock\": %zu, \"matches_gpu\": %zu, "
         "\"rules_matching\": %zu, \"events_stock\": %zu, \"events_gpu\": %zu, "
         "\"same_matches\": %s, \"same_events\": %s, \"arenas\": %llu}\n",
         n, rs, rg, done_s, done_g, a.n_m, b.n_m, rules_matching, a.n_e, b.n_e,
         same_matches ? "true" : "false", same_events ? "true" : "false",
         (unsigned long long) yr_gpu_scanner_batch_arenas(gs));
  yr_gpu_scanner_destroy(gs);
  yr_gpu_rules_destroy(gr);
  yr_rules_destroy(rules);
  yr_compiler_destroy(comp);
  yr_finalize();
  return (rs == rg && done_s == done_g && same_matches && same_events) ? 0 : 1;
}
