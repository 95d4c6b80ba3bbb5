/* The older macro names over the stand-in R.h. */
#ifndef HPN_RSHIM_RDEFINES_H
#define HPN_RSHIM_RDEFINES_H
#include "R.h"
#define NEW_INTEGER(n) allocVector(INTSXP, (long)(n))
#define NEW_NUMERIC(n) allocVector(REALSXP, (long)(n))
#define INTEGER_POINTER(x) INTEGER(x)
#define CHARACTER_VALUE(x) ((const char *)((SEXP *)(x)->data)[0]->data)
#endif
