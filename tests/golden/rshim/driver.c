/* Calls qsort_hash_count(fq1, fq2) as R's .Call would and dumps every element of the list it returns: element i (0-based) goes to
 * the file e<i>.bin in the working directory as its raw int or double cells; "elements <n>" goes to standard output.
 *   driver FQ1 [FQ2] */
#include <stdio.h>

#include "Rdefines.h"

SEXP qsort_hash_count(SEXP fq1, SEXP fq2);

static SEXP string_value(const char *s)
{
    SEXP v = allocVector(STRSXP, 1);
    SET_STRING_ELT(v, 0, mkChar(s));
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 64;
    SEXP list = qsort_hash_count(string_value(argv[1]), string_value(argc > 2 ? argv[2] : ""));
    for (long i = 0; i < list->length; ++i) {
        SEXP e = ((SEXP *)list->data)[i];
        char name[32];
        snprintf(name, sizeof name, "e%ld.bin", i);
        FILE *f = fopen(name, "wb");
        if (!f) return 65;
        fwrite(e->data, e->type == REALSXP ? sizeof(double) : sizeof(int), (size_t)e->length, f);
        fclose(f);
    }
    printf("elements %ld\n", list->length);
    return 0;
}
