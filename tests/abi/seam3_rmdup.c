/* seam3_rmdup.c -- the INTEGRATION.md "Seam 3's rmdup" stub as a C99 program: `samtools rmdup`'s survivors, their order and its
 * writer's cuts through hpn_bam_rmdup_*.
 *
 * The file's BGZF blocks are listed on the host (plain C over the 18-byte headers), inflated on the device in one call
 * (hpn_bgzf_inflate_dev) and indexed in place (hpn_bam_raw_index_dev); the header's length and its number of targets come from
 * zlib's gzread over the same file (BGZF is multi-member gzip).  The @RG table is the caller's: argv[3] libraries, then pairs of
 * ID and library number.  Then one session: _begin, _add_raw_dev, _finish, _counts, _order, and _emit in slices of argv[2]
 * records (0: all).
 * Output: "records N out M payload P", "order i0 i1 ...", per library "lib L checked removed first", per target with records
 * "target T unmatched", and per closed block "block LEN CRC32" -- what bam_write1 would put into every BGZF block behind the
 * header.  tests/test_rmdup_abi_c.py compiles this with  gcc -std=c99 -pedantic -Wall -Werror  and compares the lines with
 * tests/rmdup_ref.py.
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

static long header_length(const char *path, int32_t *targets)
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
    *targets = n_ref;
    for (t = 0; t < n_ref; ++t) {
        if (gzread(f, &l_name, 4) != 4 || gzseek(f, l_name + 4, SEEK_CUR) < 0) {
            gzclose(f);
            return -1;
        }
        at += 8 + l_name;
    }
    gzclose(f);
    return at;
}

int main(int argc, char **argv)
{
    hpn_ctx *ctx = NULL;
    FILE *f;
    uint8_t *file, *d_comp = NULL, *d_raw = NULL;
    hpn_bgzf_block *blocks, *d_blocks = NULL;
    uint32_t *d_status = NULL, *order;
    long size, hl, o;
    uint64_t n_blocks = 0, out = 0, first_block = 0, k, slice, first;
    uint32_t first_off = 0;
    hpn_raw_info raw;
    hpn_rmdup_info si;
    hpn_rmdup_result res;
    hpn_rmdup_lib *libs;
    hpn_rmdup_target *targets;
    const char *ids[64];
    uint32_t lib_of_id[64], n_ids = 0, n_libs = 1, l;
    int32_t n_ref = 0, t;
    void *p;
    int rc;
    if (argc < 2) return 2;
    slice = argc > 2 && strtoull(argv[2], NULL, 10) ? (uint64_t)strtoull(argv[2], NULL, 10) : ~(uint64_t)0;
    if (argc > 3) n_libs = (uint32_t)strtoul(argv[3], NULL, 10);
    for (rc = 4; rc + 1 < argc && n_ids < 64; rc += 2) ids[n_ids] = argv[rc], lib_of_id[n_ids++] = (uint32_t)strtoul(argv[rc + 1], NULL, 10);
    if ((hl = header_length(argv[1], &n_ref)) < 0 || !(f = fopen(argv[1], "rb"))) return 2;
    fseek(f, 0, SEEK_END);
    size = ftell(f);
    fseek(f, 0, SEEK_SET);
    file = (uint8_t *)malloc((size_t)size + 64);
    blocks = (hpn_bgzf_block *)malloc(((size_t)size / 26 + 1) * sizeof *blocks);
    if (!file || !blocks || fread(file, 1, (size_t)size, f) != (size_t)size) return 2;
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
    if ((rc = hpn_ctx_create(0, &ctx)) != HPN_OK) return fail(NULL, "hpn_ctx_create", rc);
    if ((rc = hpn_bam_rmdup_begin(ctx, n_ref, n_ids, ids, lib_of_id, n_libs)) != HPN_OK) return fail(ctx, "hpn_bam_rmdup_begin", rc);
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
            if ((rc = hpn_bam_rmdup_add_raw_dev(ctx, d_raw, &si)) != HPN_OK) return fail(ctx, "hpn_bam_rmdup_add_raw_dev", rc);
            if (si.bad_record >= 0) {
                printf("outside record %lld refID %d pos %d reason %u\n", (long long)si.bad_record, si.bad_tid, si.bad_pos, si.reason);
                return 0;
            }
        }
    }
    if ((rc = hpn_bam_rmdup_finish(ctx, &res)) != HPN_OK) return fail(ctx, "hpn_bam_rmdup_finish", rc);
    if (res.bad_record >= 0) {
        printf("outside record %lld refID %d pos %d reason %u\n", (long long)res.bad_record, res.bad_tid, res.bad_pos, res.reason);
        return 0;
    }
    printf("records %llu out %llu payload %llu\n", (unsigned long long)res.n_records, (unsigned long long)res.n_out, (unsigned long long)res.payload_bytes);
    order = (uint32_t *)malloc(((size_t)res.n_out + 1) * 4);
    libs = (hpn_rmdup_lib *)malloc((size_t)n_libs * sizeof *libs);
    targets = (hpn_rmdup_target *)malloc(((size_t)n_ref + 1) * sizeof *targets);
    if (!order || !libs || !targets) return 2;
    if ((rc = hpn_bam_rmdup_order(ctx, order, res.n_out)) != HPN_OK) return fail(ctx, "hpn_bam_rmdup_order", rc);
    if ((rc = hpn_bam_rmdup_counts(ctx, libs, targets)) != HPN_OK) return fail(ctx, "hpn_bam_rmdup_counts", rc);
    printf("order");
    for (k = 0; k < res.n_out; ++k) printf(" %u", order[k]);
    printf("\n");
    for (l = 0; l < n_libs; ++l)
        printf("lib %u %llu %llu %lld\n", l, (unsigned long long)libs[l].checked, (unsigned long long)libs[l].removed, (long long)libs[l].first);
    for (t = 0; t <= n_ref; ++t)
        if (targets[t].has_records) printf("target %d %llu\n", t, (unsigned long long)targets[t].unmatched);
    for (first = 0;;) {
        const uint64_t left = res.n_out - first, cnt = left < slice ? left : slice;
        const int last = cnt == left;
        hpn_split_info info;
        hpn_split_block *bl;
        uint64_t nb = 0;
        if ((rc = hpn_bam_rmdup_emit(ctx, first, cnt, last, &info)) != HPN_OK) return fail(ctx, "hpn_bam_rmdup_emit", rc);
        bl = (hpn_split_block *)malloc(((size_t)info.n_blocks + 1) * sizeof *bl);
        if (!bl) return 2;
        if ((rc = hpn_bam_rmdup_blocks(ctx, 0, bl, info.n_blocks, &nb)) != HPN_OK) return fail(ctx, "hpn_bam_rmdup_blocks", rc);
        for (k = 0; k < nb; ++k) printf("block %u %08x\n", bl[k].len, bl[k].crc);
        free(bl);
        first += cnt;
        if (last) break;
    }
    free(order), free(libs), free(targets), free(blocks), free(file);
    if (d_comp) hpn_dev_free(ctx, d_comp), hpn_dev_free(ctx, d_raw), hpn_dev_free(ctx, d_blocks), hpn_dev_free(ctx, d_status);
    hpn_ctx_destroy(ctx);
    return 0;
}
