/* seam3_view.c -- the INTEGRATION.md "Seam 3's view" stub as a C99 program: `samtools view`'s filters, its count and its SAM text
 * through hpn_bam_view_*.
 *
 * The file's BGZF blocks are listed on the host (plain C over the 18-byte headers), inflated on the device in one call
 * (hpn_bgzf_inflate_dev) and indexed in place (hpn_bam_raw_index_dev); the header's length and the targets' names come from
 * zlib's gzread over the same file (BGZF is multi-member gzip).  One session: _begin, _add_raw_dev, _finish, and for text
 * _text_emit / _text_dev in slices of SLICE records (0: all).
 *   seam3_view EMIT FLAG_OFF SLICE in.bam          EMIT: 1 text, 2 the count only
 * Output: "records N kept M text T", then for text the lines themselves; or "outside record R refID T pos P reason N" for the
 * first record the session cannot take.  tests/test_view_abi_c.py compiles this with  gcc -std=c99 -pedantic -Wall -Werror  and
 * compares the output with tests/view_ref.py.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <zlib.h>

#include "hpngs.h"

static int fail(hpn_ctx *c, const char *what, int rc)
{
    fprintf(stderr, "%s: %s (%s)\n", what, hpn_strerror(rc), c ? hpn_ctx_last_error(c) : "-");
    return 1;
}

static char *names;
static uint32_t *name_off;
static int32_t n_targets;

static long header_length(const char *path)
{
    gzFile f = gzopen(path, "rb");
    char magic[4];
    int32_t l_text, n_ref, l_name, t;
    long at = 12;
    if (!f) return -1;
    if (gzread(f, magic, 4) != 4 || memcmp(magic, "BAM\1", 4) != 0 || gzread(f, &l_text, 4) != 4 || gzseek(f, l_text, SEEK_CUR) < 0 ||
        gzread(f, &n_ref, 4) != 4) {
        gzclose(f);
        return -1;
    }
    at += l_text;
    n_targets = n_ref;
    name_off = (uint32_t *)calloc((size_t)n_ref + 1, 4);
    names = (char *)malloc(1);
    if (!name_off || !names) return -1;
    for (t = 0; t < n_ref; ++t) {
        int32_t l_ref;
        if (gzread(f, &l_name, 4) != 4 || l_name < 1 || !(names = (char *)realloc(names, (size_t)name_off[t] + (size_t)l_name + 1)) ||
            gzread(f, names + name_off[t], (unsigned)l_name) != l_name || gzread(f, &l_ref, 4) != 4) {
            gzclose(f);
            return -1;
        }
        name_off[t + 1] = name_off[t] + (uint32_t)strlen(names + name_off[t]);
        at += 8 + l_name;
    }
    gzclose(f);
    return at;
}

/* the file into the session; 0 done, 1 an error (said), 2 a record outside the domain (printed) */
static int add_file(hpn_ctx *ctx, const char *path, uint32_t emit, uint32_t flag_off)
{
    FILE *f;
    uint8_t *file, *d_comp, *d_raw;
    hpn_bgzf_block *blocks, *d_blocks;
    uint32_t *d_status;
    long size, hl, o;
    uint64_t n_blocks = 0, out = 0, first_block = 0;
    uint32_t first_off = 0;
    hpn_raw_info raw;
    hpn_view_info mi;
    hpn_view_opts vo;
    void *p;
    int rc, end = 0;
    if ((hl = header_length(path)) < 0 || !(f = fopen(path, "rb"))) return fail(NULL, path, HPN_E_ARG);
    memset(&vo, 0, sizeof vo);
    vo.emit = emit, vo.flag_off = flag_off, vo.n_targets = n_targets, vo.target_names = names, vo.target_name_off = name_off;
    if ((rc = hpn_bam_view_begin(ctx, &vo)) != HPN_OK) return fail(ctx, "hpn_bam_view_begin", rc);
    fseek(f, 0, SEEK_END);
    size = ftell(f);
    fseek(f, 0, SEEK_SET);
    file = (uint8_t *)malloc((size_t)size + 64);
    blocks = (hpn_bgzf_block *)malloc(((size_t)size / 26 + 1) * sizeof *blocks);
    if (!file || !blocks || fread(file, 1, (size_t)size, f) != (size_t)size) return fail(NULL, path, HPN_E_ARG);
    fclose(f);
    memset(file + size, 0, 64);
    /* the block table; blocks that hold nothing but the header are left out, the first record's offset is inside the first kept one */
    for (o = 0; o + 18 <= size;) {
        const uint32_t bsize = (uint32_t)(file[o + 16] | file[o + 17] << 8) + 1u, xlen = (uint32_t)(file[o + 10] | file[o + 11] << 8);
        uint32_t isize;
        memcpy(&isize, file + o + bsize - 4, 4);
        if ((uint64_t)hl >= out + isize && n_blocks == 0) {
            hl -= (long)isize;              /* a block of the header alone */
        } else if (isize) {
            if (n_blocks == 0) first_off = (uint32_t)hl, first_block = (uint64_t)o;
            blocks[n_blocks].in_off = (uint64_t)o - first_block + 12u + xlen;
            blocks[n_blocks].in_len = bsize - xlen - 20u;
            blocks[n_blocks].out_len = isize;
            blocks[n_blocks].out_off = out;
            out += isize, ++n_blocks;
        }
        o += (long)bsize;
    }
    if (n_blocks) {
        const size_t comp = (size_t)size - (size_t)first_block + 64;
        if ((rc = hpn_dev_malloc(ctx, comp, &p)) != HPN_OK) return fail(ctx, "hpn_dev_malloc", rc);
        d_comp = (uint8_t *)p;
        if ((rc = hpn_dev_malloc(ctx, (size_t)out + 64, &p)) != HPN_OK) return fail(ctx, "hpn_dev_malloc", rc);
        d_raw = (uint8_t *)p;
        if ((rc = hpn_dev_malloc(ctx, (size_t)n_blocks * sizeof *blocks, &p)) != HPN_OK) return fail(ctx, "hpn_dev_malloc", rc);
        d_blocks = (hpn_bgzf_block *)p;
        if ((rc = hpn_dev_malloc(ctx, (size_t)n_blocks * 4, &p)) != HPN_OK) return fail(ctx, "hpn_dev_malloc", rc);
        d_status = (uint32_t *)p;
        if ((rc = hpn_memcpy_h2d(ctx, d_comp, file + first_block, comp)) != HPN_OK) return fail(ctx, "hpn_memcpy_h2d", rc);
        if ((rc = hpn_memcpy_h2d(ctx, d_blocks, blocks, (size_t)n_blocks * sizeof *blocks)) != HPN_OK) return fail(ctx, "hpn_memcpy_h2d", rc);
        if ((rc = hpn_ctx_sync(ctx)) != HPN_OK) return fail(ctx, "hpn_ctx_sync", rc);
        if ((rc = hpn_bgzf_inflate_dev(ctx, d_comp, d_blocks, n_blocks, d_raw, d_status)) != HPN_OK) return fail(ctx, "hpn_bgzf_inflate_dev", rc);
        if ((rc = hpn_bam_raw_index_dev(ctx, d_raw, d_blocks, n_blocks, first_off, d_status, &raw)) != HPN_OK)
            return fail(ctx, "hpn_bam_raw_index_dev", rc);
        if ((raw.flags & 3u) || raw.tail_bytes) return fail(ctx, "the record index refuses the file", HPN_E_DOMAIN);
        if (raw.n_records) {
            if ((rc = hpn_bam_view_add_raw_dev(ctx, d_raw, &mi)) != HPN_OK) return fail(ctx, "hpn_bam_view_add_raw_dev", rc);
            if (mi.bad_record >= 0) {
                printf("outside record %lld refID %d pos %d reason %u\n", (long long)mi.bad_record, mi.bad_tid, mi.bad_pos, mi.reason);
                end = 2;
            }
        }
        hpn_dev_free(ctx, d_comp), hpn_dev_free(ctx, d_raw), hpn_dev_free(ctx, d_blocks), hpn_dev_free(ctx, d_status);
    }
    free(blocks), free(file);
    return end;
}

int main(int argc, char **argv)
{
    hpn_ctx *ctx = NULL;
    uint64_t slice, first;
    hpn_view_result res;
    uint32_t emit;
    int rc;
    if (argc != 5) return 2;
    emit = (uint32_t)atoi(argv[1]);
    slice = (uint64_t)strtoull(argv[3], NULL, 10);
    if (!slice) slice = ~(uint64_t)0;
    if ((rc = hpn_ctx_create(0, &ctx)) != HPN_OK) return fail(NULL, "hpn_ctx_create", rc);
    rc = add_file(ctx, argv[4], emit, (uint32_t)strtoul(argv[2], NULL, 0));
    if (rc == 2) return 0;
    if (rc) return 1;
    if ((rc = hpn_bam_view_finish(ctx, &res)) != HPN_OK) return fail(ctx, "hpn_bam_view_finish", rc);
    printf("records %llu kept %llu text %llu\n", (unsigned long long)res.n_records, (unsigned long long)res.n_out, (unsigned long long)res.text_bytes);
    for (first = 0; emit == HPN_VIEW_TEXT;) {
        hpn_view_text_info ti;
        const uint8_t *d = NULL;
        uint64_t n = 0;
        char *host;
        if ((rc = hpn_bam_view_text_emit(ctx, first, slice, &ti)) != HPN_OK) return fail(ctx, "hpn_bam_view_text_emit", rc);
        if ((rc = hpn_bam_view_text_dev(ctx, &d, &n)) != HPN_OK) return fail(ctx, "hpn_bam_view_text_dev", rc);
        host = (char *)malloc((size_t)n + 1);
        if (!host) return 2;
        if (n && ((rc = hpn_memcpy_d2h(ctx, host, d, (size_t)n)) != HPN_OK || (rc = hpn_ctx_sync(ctx)) != HPN_OK)) return fail(ctx, "hpn_memcpy_d2h", rc);
        fwrite(host, 1, (size_t)n, stdout);
        free(host);
        first += ti.n_records;
        if (first >= res.n_out) break;
    }
    free(names), free(name_off);
    hpn_ctx_destroy(ctx);
    return 0;
}
