/* burst_archive.c -- the burst archive (.brs) in C (burst_archive.h).  Little-endian, as the hosts an MI355X ships in are: the header
 * is written and read field by field through memcpy at fixed offsets, never as a struct (its 64-bit fields lie at multiples of 4).
 *
 *     0 magic "ADSBBRS1" | 8 u32 version 1 | 12 u32 kind | 16 u32 sample_bytes | 20 u64 n_units | 28 u64 M | 36 f32 threshold
 *     | 40 u32 lead | 44 u32 hang | 48 u64 n_bursts | 56 u64 payload_bytes | 64 the table, 16 bytes a record | 64 + 16 B the payload */
#include "burst_archive.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char brs_magic[8] = {'A', 'D', 'S', 'B', 'B', 'R', 'S', '1'};
#define BRS_VERSION 1u

uint32_t brs_sample_bytes(uint32_t kind)
{
    switch (kind) {
    case BRS_KIND_INT8_IQ:
        return 2;
    case BRS_KIND_PACKED12_REAL:
        return 3;
    case BRS_KIND_UINT16_REAL:
    case BRS_KIND_INT16_IQ:
    case BRS_KIND_FLOAT32_POWER:
        return 4;
    case BRS_KIND_FLOAT32_IQ:
        return 8;
    default:
        return 0;
    }
}

uint32_t brs_units_per_power_sample(uint32_t kind) { return kind == BRS_KIND_UINT16_REAL || kind == BRS_KIND_PACKED12_REAL ? 2 : 1; }

/* The layout of the archive's kind.  Kind 12's is the 12-bit one, what adsb_gather_pack12_layout gives (tests hold the two together):
 * the table is checked as a uint16 capture's is (adsb_gather_layout at 4 bytes per power sample, the one library call this file makes:
 * it builds into a stand-alone program that restates it), then piece i takes 12 ceil((hi - lo) / 4) bytes from a multiple of 16 on. */
static long brs_layout(const brs_archive *a, uint64_t *offsets, uint64_t *total)
{
    if (a->kind != BRS_KIND_PACKED12_REAL)
        return adsb_gather_layout(a->m, (int)a->sample_bytes, a->bursts, (size_t)a->n_bursts, offsets, total);
    if (adsb_gather_layout(a->m, 4, a->bursts, (size_t)a->n_bursts, NULL, NULL) != 0)
        return -1;
    uint64_t off = 0;
    for (uint64_t i = 0; i < a->n_bursts; i++) {
        const uint64_t lo = 28ull * a->bursts[i].begin, hi = 28ull * a->bursts[i].end < a->m ? 28ull * a->bursts[i].end : a->m;
        if (offsets)
            offsets[i] = off;
        off = (off + 12 * ((hi - lo + 3) / 4) + 15) & ~(uint64_t)15;
    }
    if (offsets)
        offsets[a->n_bursts] = off;
    *total = off;
    return 0;
}

uint64_t brs_piece_units(const brs_archive *a, uint64_t i)
{
    const uint64_t lo = 28ull * a->bursts[i].begin, hi = 28ull * a->bursts[i].end < a->m ? 28ull * a->bursts[i].end : a->m;
    if (a->kind == BRS_KIND_PACKED12_REAL)
        return 8 * ((hi - lo + 3) / 4);
    return brs_units_per_power_sample(a->kind) * (hi - lo);
}

static void put32(unsigned char *h, size_t at, uint32_t v) { memcpy(h + at, &v, 4); }
static void put64(unsigned char *h, size_t at, uint64_t v) { memcpy(h + at, &v, 8); }
static uint32_t get32(const unsigned char *h, size_t at)
{
    uint32_t v;
    memcpy(&v, h + at, 4);
    return v;
}
static uint64_t get64(const unsigned char *h, size_t at)
{
    uint64_t v;
    memcpy(&v, h + at, 8);
    return v;
}

/* the payload from memory (spool NULL) or from the start of a file that holds it */
static int brs_write_from(const char *path, const brs_archive *a, FILE *spool, char *why, size_t cap)
{
    uint64_t total = 0;
    if (brs_sample_bytes(a->kind) == 0 || brs_sample_bytes(a->kind) != a->sample_bytes) {
        snprintf(why, cap, "kind %u with sample_bytes %u: no format of the archive's", a->kind, a->sample_bytes);
        return -1;
    }
    if (brs_layout(a, NULL, &total) != 0) {
        snprintf(why, cap, "%s", adsb_last_error(NULL));
        return -1;
    }
    if (total != a->payload_bytes) {
        snprintf(why, cap, "the payload has %llu bytes, the table's layout %llu", (unsigned long long)a->payload_bytes, (unsigned long long)total);
        return -1;
    }
    unsigned char h[BRS_HEADER_BYTES];
    memset(h, 0, sizeof h);
    memcpy(h, brs_magic, 8);
    put32(h, 8, BRS_VERSION), put32(h, 12, a->kind), put32(h, 16, a->sample_bytes);
    put64(h, 20, a->n_units), put64(h, 28, a->m);
    memcpy(h + 36, &a->threshold, 4);
    put32(h, 40, a->lead), put32(h, 44, a->hang);
    put64(h, 48, a->n_bursts), put64(h, 56, total);
    FILE *f = fopen(path, "wb");
    if (!f) {
        snprintf(why, cap, "cannot create: %s", strerror(errno));
        return -1;
    }
    int ok = fwrite(h, 1, sizeof h, f) == sizeof h;
    ok = ok && (a->n_bursts == 0 || fwrite(a->bursts, sizeof(adsb_burst), (size_t)a->n_bursts, f) == (size_t)a->n_bursts);
    if (!spool) {
        ok = ok && (total == 0 || fwrite(a->payload, 1, (size_t)total, f) == (size_t)total);
    } else {
        static unsigned char block[1 << 16];
        ok = ok && fflush(spool) == 0 && fseeko(spool, 0, SEEK_SET) == 0;
        for (uint64_t left = total; ok && left;) {
            const size_t want = left < sizeof block ? (size_t)left : sizeof block;
            ok = fread(block, 1, want, spool) == want && fwrite(block, 1, want, f) == want;
            left -= want;
        }
    }
    if (fclose(f) != 0 || !ok) {
        snprintf(why, cap, "cannot write: %s", strerror(errno));
        return -1;
    }
    return 0;
}

int brs_write(const char *path, const brs_archive *a, char *why, size_t cap) { return brs_write_from(path, a, NULL, why, cap); }

int brs_write_spooled(const char *path, const brs_archive *a, FILE *spool, char *why, size_t cap)
{
    if (!spool) {
        snprintf(why, cap, "no spool file to take the payload from");
        return -1;
    }
    return brs_write_from(path, a, spool, why, cap);
}

int brs_read(const char *path, brs_archive *a, char *why, size_t cap)
{
    memset(a, 0, sizeof *a);
    FILE *f = fopen(path, "rb");
    if (!f) {
        snprintf(why, cap, "cannot open: %s", strerror(errno));
        return -1;
    }
    unsigned char h[BRS_HEADER_BYTES];
    const size_t got = fread(h, 1, sizeof h, f);
    long long size = -1;
    if (fseeko(f, 0, SEEK_END) == 0)
        size = (long long)ftello(f);
    int rc = -1;
    if (got != sizeof h || size < (long long)sizeof h) {
        snprintf(why, cap, "%zu bytes are no burst archive: the header alone has %d", got, BRS_HEADER_BYTES);
    } else if (memcmp(h, brs_magic, 8) != 0) {
        snprintf(why, cap, "bad magic: no burst archive");
    } else if (get32(h, 8) != BRS_VERSION) {
        snprintf(why, cap, "version %u: this reader knows version %u", get32(h, 8), BRS_VERSION);
    } else if (brs_sample_bytes(get32(h, 12)) == 0 || brs_sample_bytes(get32(h, 12)) != get32(h, 16)) {
        snprintf(why, cap, "kind %u with sample_bytes %u: no format this reader knows", get32(h, 12), get32(h, 16));
    } else {
        a->kind = get32(h, 12), a->sample_bytes = get32(h, 16);
        a->n_units = get64(h, 20), a->m = get64(h, 28);
        memcpy(&a->threshold, h + 36, 4);
        a->lead = get32(h, 40), a->hang = get32(h, 44);
        a->n_bursts = get64(h, 48), a->payload_bytes = get64(h, 56);
        const uint64_t rest = (uint64_t)size - sizeof h;
        const uint64_t m_most = brs_units_per_power_sample(a->kind) == 2 ? 2 * (a->n_units / 4) : a->n_units;
        if (a->m > m_most) {
            snprintf(why, cap, "M = %llu power samples are more than the capture's %llu samples make", (unsigned long long)a->m,
                     (unsigned long long)a->n_units);
        } else if (a->n_bursts > rest / sizeof(adsb_burst)) {
            snprintf(why, cap, "the file is too short for its table of %llu bursts", (unsigned long long)a->n_bursts);
        } else if (rest - a->n_bursts * sizeof(adsb_burst) != a->payload_bytes) {
            snprintf(why, cap, "the payload has %llu bytes, the header says %llu", (unsigned long long)(rest - a->n_bursts * sizeof(adsb_burst)),
                     (unsigned long long)a->payload_bytes);
        } else {
            /* one block: the table, the payload (16-byte aligned: 16 B bytes behind an aligned start), the offsets */
            const size_t body = (size_t)rest, off_bytes = ((size_t)a->n_bursts + 1) * sizeof(uint64_t);
            if (posix_memalign(&a->mem, 16, ((body + 15) & ~(size_t)15) + off_bytes + 16) != 0) {
                a->mem = NULL;
                snprintf(why, cap, "out of memory for the archive's %zu bytes", body);
            } else if (fseeko(f, (off_t)sizeof h, SEEK_SET) != 0 || fread(a->mem, 1, body, f) != body) {
                snprintf(why, cap, "cannot read the archive's %zu bytes: %s", body, strerror(errno));
            } else {
                a->bursts = (const adsb_burst *)a->mem;
                a->payload = (const unsigned char *)a->mem + a->n_bursts * sizeof(adsb_burst);
                a->offsets = (uint64_t *)((unsigned char *)a->mem + ((body + 15) & ~(size_t)15));
                uint64_t total = 0;
                if (brs_layout(a, a->offsets, &total) != 0)
                    snprintf(why, cap, "%s", adsb_last_error(NULL));
                else if (total != a->payload_bytes)
                    snprintf(why, cap, "the payload has %llu bytes, the table's layout %llu", (unsigned long long)a->payload_bytes,
                             (unsigned long long)total);
                else
                    rc = 0;
            }
        }
    }
    fclose(f);
    if (rc != 0)
        brs_free(a);
    return rc;
}

void brs_free(brs_archive *a)
{
    free(a->mem);
    memset(a, 0, sizeof *a);
}
