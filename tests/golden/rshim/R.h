/* A stand-in for R's C interface, just wide enough to compile a .Call entry point outside R and look at the list it returns
 * (tests/golden/make_golden_rqc.py).  Nothing here is R's: a value is a tagged array, protection is a no-op, attributes are
 * dropped. */
#ifndef HPN_RSHIM_R_H
#define HPN_RSHIM_R_H
#include <stdlib.h>
#include <string.h>

enum { CHARSXP = 9, INTSXP = 13, REALSXP = 14, STRSXP = 16, VECSXP = 19 };

typedef struct shim_value {
    int type;
    long length;
    void *data; /* int[], double[], char[] or struct shim_value *[] by type */
} *SEXP;

static SEXP R_NamesSymbol = 0;

static SEXP allocVector(int type, long n)
{
    SEXP v = (SEXP)malloc(sizeof *v);
    size_t each = type == INTSXP ? sizeof(int) : type == REALSXP ? sizeof(double) : sizeof(SEXP);
    v->type = type, v->length = n;
    v->data = calloc(n > 0 ? (size_t)n : 1, each);
    return v;
}

static SEXP allocMatrix(int type, int rows, int cols) { return allocVector(type, (long)rows * cols); }

static SEXP mkChar(const char *s)
{
    SEXP v = (SEXP)malloc(sizeof *v);
    v->type = CHARSXP, v->length = (long)strlen(s), v->data = strdup(s);
    return v;
}

#define PROTECT(x) (x)
#define UNPROTECT(n) ((void)(n))
#define INTEGER(x) ((int *)(x)->data)
#define REAL(x) ((double *)(x)->data)
#define SET_VECTOR_ELT(v, i, x) (((SEXP *)(v)->data)[i] = (x))
#define SET_STRING_ELT(v, i, x) (((SEXP *)(v)->data)[i] = (x))
#define setAttrib(x, name, value) ((void)(value))
#endif
