/*
 * tests/r_mock/r_mock.c -- a stand-in R runtime, TEST INFRASTRUCTURE ONLY.
 *
 * It implements exactly the R C-API entry points declared in tests/r_api_decls/ (the ones geneticscre_amd/csrc/r_shim.c
 * uses), with the semantics "Writing R Extensions" documents for them (sections 5.9 "Handling R objects in C", 5.10
 * "Interface functions .C and .Call", 6.1 "Memory allocation", 6.2 "Error signaling", 5.4 "Registering native routines"),
 * so that the shim can be linked into one shared object with this file and EXECUTED from the tests through ctypes.
 * Nothing here comes from R's sources: it is our reading of the manual.  What it is not: R.  There is no garbage
 * collector (objects live until mock_reset), Rf_coerceVector knows the int <-> double conversions only, and nothing is
 * evaluated.  A pass under this runtime shows that the shim's marshalling, registration, protect balance and error
 * roads do what its source says; it does not show that R agrees with our reading.
 *
 * Second half: a small exported driver for ctypes (mock_*): build argument objects from caller-supplied column-major
 * storage, call a registered routine by name through the function pointer the shim registered (as .Call would), walk
 * a result, read the protect depth / allocation counters, arm an allocation fault.
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>

#include <math.h>
#include <setjmp.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NILSXP 0
#define CHARSXP 9

struct SEXPREC {
  int type;
  R_xlen_t n;
  void* data;                          /* int / double / SEXP elements, or the bytes of a CHARSXP */
  SEXP names, dim, row_names, klass;   /* the four attributes the shim and its callers use; NULL = not set */
};

static struct SEXPREC g_nil = {NILSXP, 0, NULL, NULL, NULL, NULL, NULL};
static struct SEXPREC g_blank = {CHARSXP, 0, (void*)"", NULL, NULL, NULL, NULL};   /* what a fresh STRSXP holds */
static struct SEXPREC g_sym_names, g_sym_row_names, g_sym_class;
SEXP R_NamesSymbol = &g_sym_names, R_RowNamesSymbol = &g_sym_row_names, R_ClassSymbol = &g_sym_class;
int R_NaInt = -2147483647 - 1;

/* ---- errors: a longjmp to the innermost handler, the message kept for the test ------------------------------------ */
static jmp_buf* g_top;   /* innermost handler: R_ExecWithCleanup or the driver's mock_call */
static char g_errmsg[1024];

void Rf_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_errmsg, sizeof g_errmsg, fmt, ap);
  va_end(ap);
  if (g_top) longjmp(*g_top, 1);
  fprintf(stderr, "r_mock: Rf_error outside a call: %s\n", g_errmsg);
  abort();
}

/* ---- allocation: every object and every R_alloc block is kept on one list until mock_reset ------------------------- */
struct block {
  struct block* next;
};
static struct block* g_blocks;
static long g_allocs;    /* allocations since the library was loaded */
static long g_fail_in;   /* > 0: the g_fail_in-th allocation from now on fails (one shot) */

static void* arena(size_t bytes) {
  g_allocs++;
  if (g_fail_in > 0 && --g_fail_in == 0) Rf_error("cannot allocate memory (stand-in allocation fault)");
  struct block* b = (struct block*)calloc(1, sizeof(struct block) + 16 + bytes);
  if (!b) Rf_error("cannot allocate memory");
  b->next = g_blocks;
  g_blocks = b;
  return (char*)b + 16;   /* (sizeof(struct block) <= 16: the payload stays 16-byte aligned) */
}

static size_t elt_size(SEXPTYPE t) {
  switch (t) {
    case INTSXP: return sizeof(int);
    case REALSXP: return sizeof(double);
    case STRSXP:
    case VECSXP: return sizeof(SEXP);
    default: Rf_error("r_mock: allocVector of type %u is not implemented", t);
  }
}

SEXP Rf_allocVector(SEXPTYPE t, R_xlen_t n) {
  if (n < 0) Rf_error("negative length vectors are not allowed");
  const size_t el = elt_size(t);
  SEXP s = (SEXP)arena(sizeof *s + 16 + (size_t)n * el);
  s->type = (int)t;
  s->n = n;
  s->data = (char*)s + ((sizeof *s + 15) & ~(size_t)15);
  if (t == STRSXP)
    for (R_xlen_t i = 0; i < n; i++) ((SEXP*)s->data)[i] = &g_blank;
  if (t == VECSXP)
    for (R_xlen_t i = 0; i < n; i++) ((SEXP*)s->data)[i] = &g_nil;
  return s;
}

SEXP Rf_allocMatrix(SEXPTYPE t, int nrow, int ncol) {
  if (nrow < 0 || ncol < 0) Rf_error("negative extents to matrix");
  SEXP s = Rf_allocVector(t, (R_xlen_t)nrow * ncol);
  SEXP d = Rf_allocVector(INTSXP, 2);
  ((int*)d->data)[0] = nrow;
  ((int*)d->data)[1] = ncol;
  s->dim = d;
  return s;
}

SEXP Rf_mkChar(const char* c) {
  const size_t len = strlen(c);
  SEXP s = (SEXP)arena(sizeof *s + len + 1);
  s->type = CHARSXP;
  s->n = (R_xlen_t)len;
  s->data = (char*)s + sizeof *s;
  memcpy(s->data, c, len + 1);
  return s;
}

SEXP Rf_mkString(const char* c) {
  SEXP s = Rf_allocVector(STRSXP, 1);
  ((SEXP*)s->data)[0] = Rf_mkChar(c);
  return s;
}

char* R_alloc(size_t n, int size) { return (char*)arena(n * (size_t)size); }

/* ---- protection: a counter a test can read (there is no collector to protect from) --------------------------------- */
static int g_protect;
SEXP Rf_protect(SEXP s) {
  g_protect++;
  return s;
}
void Rf_unprotect(int n) {
  if (n > g_protect) Rf_error("unprotect(): only %d protected items", g_protect);
  g_protect -= n;
}

/* ---- accessors: a wrong type is an R error, as in R ---------------------------------------------------------------- */
int TYPEOF(SEXP s) { return s->type; }
R_xlen_t XLENGTH(SEXP s) { return s->n; }
int* INTEGER(SEXP s) {
  if (s->type != INTSXP) Rf_error("INTEGER() can only be applied to a 'integer', not type %d", s->type);
  return (int*)s->data;
}
double* REAL(SEXP s) {
  if (s->type != REALSXP) Rf_error("REAL() can only be applied to a 'numeric', not type %d", s->type);
  return (double*)s->data;
}
const char* R_CHAR(SEXP s) {
  if (s->type != CHARSXP) Rf_error("CHAR() can only be applied to a 'CHARSXP', not type %d", s->type);
  return (const char*)s->data;
}
static SEXP* elts(SEXP s, int type, R_xlen_t i, const char* what) {
  if (s->type != type) Rf_error("%s() applied to type %d", what, s->type);
  if (i < 0 || i >= s->n) Rf_error("%s(): index %ld out of bounds (length %ld)", what, (long)i, (long)s->n);
  return (SEXP*)s->data + i;
}
SEXP VECTOR_ELT(SEXP s, R_xlen_t i) { return *elts(s, VECSXP, i, "VECTOR_ELT"); }
SEXP SET_VECTOR_ELT(SEXP s, R_xlen_t i, SEXP v) { return *elts(s, VECSXP, i, "SET_VECTOR_ELT") = v; }
SEXP STRING_ELT(SEXP s, R_xlen_t i) { return *elts(s, STRSXP, i, "STRING_ELT"); }
void SET_STRING_ELT(SEXP s, R_xlen_t i, SEXP v) {
  if (v->type != CHARSXP) Rf_error("SET_STRING_ELT(): value of type %d is not a CHARSXP", v->type);
  *elts(s, STRSXP, i, "SET_STRING_ELT") = v;
}

/* ---- attributes ---------------------------------------------------------------------------------------------------- */
static SEXP* attr_slot(SEXP s, SEXP which) {
  if (which == R_NamesSymbol) return &s->names;
  if (which == R_RowNamesSymbol) return &s->row_names;
  if (which == R_ClassSymbol) return &s->klass;
  Rf_error("r_mock: attribute symbol not implemented");
}
SEXP Rf_getAttrib(SEXP s, SEXP which) {
  SEXP v = *attr_slot(s, which);
  return v ? v : &g_nil;
}
SEXP Rf_setAttrib(SEXP s, SEXP which, SEXP v) {
  if (which == R_NamesSymbol && v->type != NILSXP && (v->type != STRSXP || v->n != s->n))
    Rf_error("'names' attribute must be a character vector of the length of the vector");
  *attr_slot(s, which) = v->type == NILSXP ? NULL : v;
  return v;
}
int Rf_nrows(SEXP s) { return s->dim ? ((int*)s->dim->data)[0] : (int)s->n; }   /* a plain vector is a column */
int Rf_ncols(SEXP s) { return s->dim ? ((int*)s->dim->data)[1] : 1; }

/* ---- coercion: integer <-> double, NA kept, dim and names kept; the same type comes back as it is ----------------- */
static int real_to_int(double d) {
  if (isnan(d) || d >= 2147483648.0 || d <= -2147483649.0) return R_NaInt;   /* (R warns: NAs introduced by coercion) */
  return (int)d;                                                             /* truncation towards zero */
}
static double int_to_real(int i) { return i == R_NaInt ? NAN : (double)i; }

SEXP Rf_coerceVector(SEXP x, SEXPTYPE t) {
  if ((SEXPTYPE)x->type == t) return x;
  if (!((x->type == INTSXP && t == REALSXP) || (x->type == REALSXP && t == INTSXP)))
    Rf_error("r_mock: coerceVector from type %d to %u is not implemented", x->type, t);
  SEXP y = Rf_allocVector(t, x->n);
  for (R_xlen_t i = 0; i < x->n; i++) {
    if (t == INTSXP) ((int*)y->data)[i] = real_to_int(((double*)x->data)[i]);
    else ((double*)y->data)[i] = int_to_real(((int*)x->data)[i]);
  }
  y->dim = x->dim;
  y->names = x->names;
  return y;
}
int Rf_asInteger(SEXP s) {
  if (s->n < 1) return R_NaInt;
  if (s->type == INTSXP) return ((int*)s->data)[0];
  if (s->type == REALSXP) return real_to_int(((double*)s->data)[0]);
  return R_NaInt;
}
double Rf_asReal(SEXP s) {
  if (s->n < 1) return NAN;
  if (s->type == INTSXP) return int_to_real(((int*)s->data)[0]);
  if (s->type == REALSXP) return ((double*)s->data)[0];
  return NAN;
}

/* ---- R_ExecWithCleanup: the cleanup runs on the normal road and on the longjmp road, then the jump goes on -------- */
static long g_exec_allocs;   /* allocations made inside the last fun() that returned normally */

SEXP R_ExecWithCleanup(SEXP (*fun)(void*), void* data, void (*cleanfun)(void*), void* cleandata) {
  jmp_buf here;
  jmp_buf* const outer = g_top;
  const long a0 = g_allocs;
  g_top = &here;
  if (setjmp(here) == 0) {
    SEXP r = fun(data);
    g_top = outer;
    g_exec_allocs = g_allocs - a0;
    cleanfun(cleandata);
    return r;
  }
  g_top = outer;
  cleanfun(cleandata);
  if (g_top) longjmp(*g_top, 1);
  fprintf(stderr, "r_mock: error outside a call: %s\n", g_errmsg);
  abort();
}

/* ---- registration: the table is recorded, .Call goes through it --------------------------------------------------- */
static const R_CallMethodDef* g_call_table;
static int g_dynamic_symbols = -1;

int R_registerRoutines(DllInfo* dll, const void* c_routines, const R_CallMethodDef* call_routines,
                       const void* fortran_routines, const void* external_routines) {
  (void)dll; (void)c_routines; (void)fortran_routines; (void)external_routines;
  g_call_table = call_routines;
  return 1;
}
Rboolean R_useDynamicSymbols(DllInfo* dll, Rboolean value) {
  (void)dll;
  const int old = g_dynamic_symbols;
  g_dynamic_symbols = (int)value;
  return old == 0 ? FALSE : TRUE;   /* symbols are looked up dynamically until a package says otherwise */
}

/* ====================================================================================================================
 * the driver (ctypes)
 * ==================================================================================================================== */
void R_init_geneticsCRE(DllInfo*);   /* the shim's initialiser: R calls R_init_<package> when it loads the object */

/* every constructor below can hit the allocation fault: outside a call that would abort, so they run under a handler
 * of their own and return NULL with the message */
#define GUARDED(expr)                \
  jmp_buf here;                      \
  jmp_buf* const outer = g_top;      \
  SEXP r = NULL;                     \
  g_top = &here;                     \
  if (setjmp(here) == 0) r = (expr); \
  g_top = outer;                     \
  return r

static SEXP ints(const int* v, long n, int nrow, int ncol) {
  SEXP s = nrow >= 0 ? Rf_allocMatrix(INTSXP, nrow, ncol) : Rf_allocVector(INTSXP, n);
  if (s->n) memcpy(s->data, v, (size_t)s->n * sizeof(int));
  return s;
}
static SEXP reals(const double* v, long n, int nrow, int ncol) {
  SEXP s = nrow >= 0 ? Rf_allocMatrix(REALSXP, nrow, ncol) : Rf_allocVector(REALSXP, n);
  if (s->n) memcpy(s->data, v, (size_t)s->n * sizeof(double));
  return s;
}
void mock_load(void) { R_init_geneticsCRE(NULL); }
SEXP mock_int_vector(const int* v, long n) { GUARDED(ints(v, n, -1, -1)); }
SEXP mock_real_vector(const double* v, long n) { GUARDED(reals(v, n, -1, -1)); }
/* `v` is the matrix as R stores it: column-major, element (r, c) at v[c * nrow + r] */
SEXP mock_int_matrix(const int* v, int nrow, int ncol) { GUARDED(ints(v, 0, nrow, ncol)); }
SEXP mock_real_matrix(const double* v, int nrow, int ncol) { GUARDED(reals(v, 0, nrow, ncol)); }
SEXP mock_string(const char* c) { GUARDED(Rf_mkString(c)); }
SEXP mock_list(long n) { GUARDED(Rf_allocVector(VECSXP, n)); }
/* lst[[name]] <- value at position i (name == NULL: no name) */
static SEXP list_set(SEXP lst, long i, const char* name, SEXP value) {
  SET_VECTOR_ELT(lst, i, value);
  if (name) {
    if (!lst->names) lst->names = Rf_allocVector(STRSXP, lst->n);
    SET_STRING_ELT(lst->names, i, Rf_mkChar(name));
  }
  return lst;
}
SEXP mock_list_set(SEXP lst, long i, const char* name, SEXP value) { GUARDED(list_set(lst, i, name, value)); }

int mock_registered_count(void) {
  int n = 0;
  while (g_call_table && g_call_table[n].name) n++;
  return n;
}
const char* mock_registered_name(int i) { return g_call_table[i].name; }
int mock_registered_nargs(int i) { return g_call_table[i].numArgs; }
int mock_dynamic_symbols(void) { return g_dynamic_symbols; }   /* -1: R_useDynamicSymbols was never called */

typedef SEXP (*fn3)(SEXP, SEXP, SEXP);
typedef SEXP (*fn4)(SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*fn39)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP,
                     SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP,
                     SEXP, SEXP, SEXP, SEXP, SEXP);

/* .Call(name, args...): the routine registered under `name`, called through the recorded pointer with the recorded
 * number of arguments.  NULL on an R error (message: mock_error_message); the protect stack is then back where it was
 * when the call began, as R leaves it. */
SEXP mock_call(const char* name, SEXP* a, int nargs) {
  const R_CallMethodDef* def = NULL;
  for (int i = 0; g_call_table && g_call_table[i].name; i++)
    if (strcmp(g_call_table[i].name, name) == 0) def = &g_call_table[i];
  g_errmsg[0] = 0;
  if (!def) {
    snprintf(g_errmsg, sizeof g_errmsg, "\"%s\" not available for .Call()", name);
    return NULL;
  }
  if (def->numArgs != nargs) {
    snprintf(g_errmsg, sizeof g_errmsg, "Incorrect number of arguments (%d), expecting %d for '%s'", nargs, def->numArgs, name);
    return NULL;
  }
  jmp_buf here;
  jmp_buf* const outer = g_top;
  const int depth = g_protect;
  SEXP volatile r = NULL;
  g_top = &here;
  if (setjmp(here) == 0) {
    switch (nargs) {
      case 3: r = ((fn3)def->fun)(a[0], a[1], a[2]); break;
      case 4: r = ((fn4)def->fun)(a[0], a[1], a[2], a[3]); break;
      case 39:
        r = ((fn39)def->fun)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14],
                             a[15], a[16], a[17], a[18], a[19], a[20], a[21], a[22], a[23], a[24], a[25], a[26], a[27], a[28],
                             a[29], a[30], a[31], a[32], a[33], a[34], a[35], a[36], a[37], a[38]);
        break;
      default: Rf_error("r_mock: calls with %d arguments are not implemented", nargs);
    }
  } else {
    r = NULL;
    g_protect = depth;
  }
  g_top = outer;
  g_fail_in = 0;
  return r;
}

const char* mock_error_message(void) { return g_errmsg; }
int mock_protect_depth(void) { return g_protect; }
long mock_alloc_count(void) { return g_allocs; }
long mock_exec_allocs(void) { return g_exec_allocs; }
void mock_fail_alloc(long nth) { g_fail_in = nth; }   /* the nth allocation from now on calls Rf_error; 0 disarms */
/* forget every object made so far (what R's collector and the end of a .Call do to objects nobody holds) */
void mock_reset(void) {
  while (g_blocks) {
    struct block* b = g_blocks;
    g_blocks = b->next;
    free(b);
  }
}

/* walking a result */
int mock_typeof(SEXP s) { return s->type; }
long mock_length(SEXP s) { return (long)s->n; }
const void* mock_data(SEXP s) { return s->data; }   /* int / double elements, or the bytes of a CHARSXP */
SEXP mock_elt(SEXP s, long i) {                     /* element of a list or of a character vector */
  return (s->type == VECSXP || s->type == STRSXP) && i >= 0 && i < s->n ? ((SEXP*)s->data)[i] : NULL;
}
SEXP mock_attr(SEXP s, const char* which) {         /* "names", "dim", "row.names", "class"; NULL = not set */
  if (strcmp(which, "names") == 0) return s->names;
  if (strcmp(which, "dim") == 0) return s->dim;
  if (strcmp(which, "row.names") == 0) return s->row_names;
  if (strcmp(which, "class") == 0) return s->klass;
  return NULL;
}
