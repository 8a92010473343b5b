/*
 * tests/r_mock/gcre_stub.c -- a recording backend for the .Call shim, TEST INFRASTRUCTURE ONLY.
 *
 * The shim (geneticscre_amd/csrc/r_shim.c) dlopen()s the library GCRE_HIP_LIB names and resolves four symbols.  This file
 * exports those four: gcre_process_paths_devices keeps a deep copy of everything it was handed and returns results a test
 * has queued, gcre_result_free counts the frees per result, gcre_device_count returns what the test set, and
 * gcre_resolve_count_locs forwards to the real libgcre_hip.so (host code, loads without a GPU).  tests/test_r_shim_host.py
 * loads the same object through ctypes and reads what was recorded (stub_*).
 */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gcre_hip.h"

static void* copy(const void* p, size_t bytes) {
  if (!p) return NULL;
  void* q = malloc(bytes ? bytes : 1);
  if (bytes) memcpy(q, p, bytes);
  return q;
}

/* ---- what the last gcre_process_paths_devices call received ------------------------------------------------------- */
static struct {
  int calls;
  int method, n_cases, n_ctrls, iterations, top_k, n_devices, devices_null;
  int devices[256];
  gcre_pp_input in;   /* every pointer is a copy owned here */
} rec;

static void free_input(void) {
  for (int l = 0; l < 6; l++) {
    free((void*)rec.in.level[l].uid_count);
    free((void*)rec.in.level[l].uid_location);
    free((void*)rec.in.level[l].signs);
  }
  for (int i = 0; i < 4; i++) free((void*)rec.in.data_inds[i]);
  free((void*)rec.in.data1);
  free((void*)rec.in.data2);
  free((void*)rec.in.value_table);
  free((void*)rec.in.perm_cases);
  memset(&rec.in, 0, sizeof rec.in);
}

/* ---- the results the next calls return ---------------------------------------------------------------------------- */
static gcre_result queued[5] = {{-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0},
                                {-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}};
static int return_code = GCRE_OK;
static char return_msg[256];
static int device_count = 1;

/* ---- frees --------------------------------------------------------------------------------------------------------- */
static gcre_result* out_base;   /* the array the last call filled: a result is known by its place in it */
static int handed_out[5], freed[5], double_frees, foreign_frees;

static void release_arrays(gcre_result* r) {
  free(r->scores);
  free(r->src);
  free(r->trg);
  free(r->cases);
  free(r->ctrls);
  free(r->null_max);
  r->scores = NULL;
  r->src = r->trg = r->cases = r->ctrls = NULL;
  r->null_max = NULL;
}

int gcre_process_paths_devices(int method, int n_cases, int n_ctrls, int iterations, int top_k, const int* devices,
                               int n_devices, const gcre_pp_input* in, gcre_result out[5], char* err, size_t errlen) {
  const size_t n = (size_t)(n_cases + n_ctrls);
  rec.calls++;
  rec.method = method;
  rec.n_cases = n_cases;
  rec.n_ctrls = n_ctrls;
  rec.iterations = iterations;
  rec.top_k = top_k;
  rec.n_devices = n_devices;
  rec.devices_null = devices == NULL;
  for (int i = 0; i < n_devices && i < 256; i++) rec.devices[i] = devices ? devices[i] : -1;
  free_input();
  rec.in = *in;
  for (int l = 0; l < 6; l++) {
    gcre_level* lv = &rec.in.level[l];
    lv->uid_count = copy(lv->uid_count, (size_t)lv->n_uids * sizeof(int32_t));
    lv->uid_location = copy(lv->uid_location, (size_t)lv->n_uids * sizeof(int64_t));
    lv->signs = copy(lv->signs, (size_t)lv->n_signs * sizeof(int32_t));
  }
  for (int i = 0; i < 4; i++) rec.in.data_inds[i] = copy(in->data_inds[i], (size_t)in->n_data_inds[i] * sizeof(int32_t));
  rec.in.data1 = copy(in->data1, (size_t)in->data1_rows * n * sizeof(int32_t));
  rec.in.data2 = copy(in->data2, (size_t)in->data2_rows * n * sizeof(int32_t));
  rec.in.value_table = copy(in->value_table, (size_t)in->vt_rows * (size_t)in->vt_cols * sizeof(double));
  rec.in.perm_cases = copy(in->perm_cases, (size_t)in->perm_rows * n * sizeof(int32_t));

  out_base = out;
  for (int i = 0; i < 5; i++) {
    memset(&out[i], 0, sizeof out[i]);
    out[i].n = -1;
    handed_out[i] = freed[i] = 0;
  }
  if (return_code != GCRE_OK) {
    if (err && errlen) snprintf(err, errlen, "%s", return_msg);
    return return_code;
  }
  for (int i = 0; i < 5; i++) {
    const gcre_result* q = &queued[i];
    if (q->n < 0) continue;
    out[i].n = q->n;
    out[i].n_perm = q->n_perm;
    out[i].scores = copy(q->scores, (size_t)q->n * sizeof(double));
    out[i].src = copy(q->src, (size_t)q->n * sizeof(int32_t));
    out[i].trg = copy(q->trg, (size_t)q->n * sizeof(int32_t));
    out[i].cases = copy(q->cases, (size_t)q->n * sizeof(int32_t));
    out[i].ctrls = copy(q->ctrls, (size_t)q->n * sizeof(int32_t));
    out[i].null_max = copy(q->null_max, (size_t)q->n_perm * sizeof(float));
    handed_out[i] = 1;
  }
  return GCRE_OK;
}

void gcre_result_free(gcre_result* r) {
  const intptr_t off = (intptr_t)r - (intptr_t)out_base;
  const long i = out_base && off >= 0 && off % (intptr_t)sizeof *r == 0 ? (long)(off / (intptr_t)sizeof *r) : -1;
  if (i < 0 || i >= 5 || !handed_out[i]) {   /* not a result this backend returned (or one with n = -1) */
    foreign_frees++;
    return;
  }
  if (++freed[i] > 1) {
    double_frees++;
    return;
  }
  release_arrays(r);
}

int gcre_device_count(void) { return device_count; }

static void* real_lib;
static int (*real_resolve)(const int32_t*, int64_t, const int32_t*, const int32_t*, const int32_t*, int64_t, int32_t*, int64_t*);
static int resolve_calls;

int gcre_resolve_count_locs(const int32_t* trg_uids, int64_t n_uids, const int32_t* keys, const int32_t* counts,
                            const int32_t* locations, int64_t n_keys, int32_t* out_count, int64_t* out_location) {
  resolve_calls++;
  if (!real_resolve) return GCRE_ERR_ARG;
  return real_resolve(trg_uids, n_uids, keys, counts, locations, n_keys, out_count, out_location);
}

/* ---- the test's side ----------------------------------------------------------------------------------------------- */
int stub_set_real_lib(const char* path) {   /* 0 = loaded and the symbol found */
  real_lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!real_lib) {
    fprintf(stderr, "gcre_stub: %s\n", dlerror());
    return -1;
  }
  *(void**)(&real_resolve) = dlsym(real_lib, "gcre_resolve_count_locs");
  return real_resolve ? 0 : -2;
}
void stub_set_device_count(int n) { device_count = n; }
void stub_set_return(int rc, const char* msg) {
  return_code = rc;
  snprintf(return_msg, sizeof return_msg, "%s", msg ? msg : "");
}
/* lst<level + 1> of the calls that follow; n = -1: a level above path_length */
void stub_queue_result(int level, int n, const double* scores, const int32_t* src, const int32_t* trg, const int32_t* cases,
                       const int32_t* ctrls, int n_perm, const float* null_max) {
  gcre_result* q = &queued[level];
  release_arrays(q);
  q->n = n;
  q->n_perm = n_perm;
  if (n < 0) return;
  q->scores = copy(scores, (size_t)n * sizeof(double));
  q->src = copy(src, (size_t)n * sizeof(int32_t));
  q->trg = copy(trg, (size_t)n * sizeof(int32_t));
  q->cases = copy(cases, (size_t)n * sizeof(int32_t));
  q->ctrls = copy(ctrls, (size_t)n * sizeof(int32_t));
  q->null_max = copy(null_max, (size_t)n_perm * sizeof(float));
}
int stub_calls(void) { return rec.calls; }
int stub_resolve_calls(void) { return resolve_calls; }
int stub_scalar(int which) {   /* 0 method, 1 n_cases, 2 n_ctrls, 3 iterations, 4 top_k, 5 n_devices, 6 devices == NULL */
  const int v[7] = {rec.method, rec.n_cases, rec.n_ctrls, rec.iterations, rec.top_k, rec.n_devices, rec.devices_null};
  return which >= 0 && which < 7 ? v[which] : -1;
}
const int* stub_devices(void) { return rec.devices; }
const gcre_pp_input* stub_input(void) { return &rec.in; }
int stub_handed_out(int level) { return handed_out[level]; }
int stub_freed(int level) { return freed[level]; }
int stub_double_frees(void) { return double_frees; }
int stub_foreign_frees(void) { return foreign_frees; }
void stub_reset_counters(void) {
  rec.calls = resolve_calls = double_frees = foreign_frees = 0;
  for (int i = 0; i < 5; i++) handed_out[i] = freed[i] = 0;
}
