/* burst_archive.h -- the burst archive (.brs) in C: what the host program's -K and -P write and -k reads.  The format, the layout of the
 * payload and the rules a reader keeps are adsbdec_amd/burst_archive.py's, word for word; the two read each other's files.
 * Part of the host program, not of the library's ABI. */
#ifndef ADSBDEC_AMD_CLI_BURST_ARCHIVE_H
#define ADSBDEC_AMD_CLI_BURST_ARCHIVE_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "adsbdec_amd.h"

#define BRS_HEADER_BYTES 64
enum { BRS_KIND_FLOAT32_IQ = 0, BRS_KIND_INT16_IQ = 2, BRS_KIND_UINT16_REAL = 4, BRS_KIND_INT8_IQ = 8, BRS_KIND_FLOAT32_POWER = 16,
       BRS_KIND_PACKED12_REAL = 12 /* a real capture's pieces as Airspy packed 12-bit samples (adsb_gather_pack12_*): sample_bytes 3 */ };

typedef struct {
    uint32_t kind, sample_bytes; /* sample_bytes: per POWER sample (brs_sample_bytes) */
    uint64_t n_units, m;         /* the capture's length in its own samples; its power samples */
    float threshold;
    uint32_t lead, hang;
    uint64_t n_bursts, payload_bytes;
    const adsb_burst *bursts;     /* n_bursts records */
    const unsigned char *payload; /* payload_bytes: what adsb_gather_device (kind 12: adsb_gather_pack12_*) wrote; from brs_read, 16-byte aligned */
    uint64_t *offsets;            /* brs_read: n_bursts + 1, piece i is payload + offsets[i] */
    void *mem;                    /* brs_read: what brs_free releases */
} brs_archive;

/* bytes per power sample of a kind (2, 3, 4, 8), or 0 for a number that is no kind */
uint32_t brs_sample_bytes(uint32_t kind);
/* the capture's own samples per power sample: 2 for uint16 real and packed 12-bit real, else 1 */
uint32_t brs_units_per_power_sample(uint32_t kind);
/* piece i's length as the batch decode call of the kind counts it: its units; kind 12: 8 ceil((hi - lo) / 4), the fill included */
uint64_t brs_piece_units(const brs_archive *a, uint64_t i);
/* 0, or -1 with the reason in why[cap].  brs_write checks the table and the payload's size by the layout of the kind first
 * (adsb_gather_layout; kind 12: adsb_gather_pack12_layout). */
int brs_write(const char *path, const brs_archive *a, char *why, size_t cap);
/* The same file with the payload taken from the first payload_bytes bytes of `spool`, a file open for reading and writing (the record
 * mode appends each piece's gathered bytes to one): a->payload is not read, and the payload is never in memory in one piece. */
int brs_write_spooled(const char *path, const brs_archive *a, FILE *spool, char *why, size_t cap);
/* The whole file into memory of the archive's own.  Refused: a file that cannot be read, another magic or version, a kind and
 * sample_bytes that do not go together, an M the capture's units cannot make, a table the kind's layout refuses, a payload of another
 * size than the layout's total. */
int brs_read(const char *path, brs_archive *a, char *why, size_t cap);
void brs_free(brs_archive *a);
#endif
