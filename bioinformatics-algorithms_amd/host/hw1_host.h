/*
 * hw1_host.h -- the host-only pieces of hw1_amd (libhw1_host.so): the reference's FASTA reader and its DOT output,
 * restated over a suffix array.  No HIP here, so the CPU test suite loads this library on machines without a GPU.
 *
 * The reference is multiple_pattern_matching/multiple_pattern_matching.cpp:
 *   hw1_read_sequences  readSequences: reading stops at the first EMPTY line (a "\r" or blank line does not stop it),
 *                       every line is trimmed of " \t\r\n" at both ends, a record is kept only when its header is
 *                       non-empty and the sequence buffer is cleared only then (lines before the first header, and
 *                       those of a bare ">" record, run into the next record's sequence).  A file that cannot be opened
 *                       prints "Cannot open file: <path>" on stderr and reads as empty (*opened = 0).
 *   hw1_terminator      the byte after reference i of n_refs: "$#@%^&!"[i] for up to 7 references, else the bytes
 *                       33..126 without A, C, G, T (90 of them) -- and past those 90, where the reference reads beyond
 *                       its list, entry i mod 90 ("hw1: unpinned regions").
 *   hw1_write_dot       printDot over the suffix tree of text: the tree is rebuilt from the suffix array and the LCP
 *                       array (Kasai) and written in the reference's pre-order, children in signed-char order; no tree
 *                       is held in memory.  Reference r is text[ref_start[r] .. ref_start[r + 1]) with its terminator
 *                       last; a leaf at p inside it is labelled "<header>:<p - start>:<p>", a leaf on a terminator "<p>".
 *                       Returns 0, or -1 when the file cannot be written (the reference writes nothing then either).
 */
#ifndef HW1_HOST_H
#define HW1_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hw1_records hw1_records;
hw1_records *hw1_read_sequences(const char *path, int *opened);
uint32_t hw1_records_count(const hw1_records *r);
const char *hw1_records_header(const hw1_records *r, uint32_t i, uint64_t *len);
const char *hw1_records_sequence(const hw1_records *r, uint32_t i, uint64_t *len);
void hw1_records_free(hw1_records *r);

int hw1_terminator(uint32_t n_refs, uint32_t i);

int hw1_write_dot(const char *path, const uint8_t *text, uint32_t n, const uint32_t *sa, uint32_t n_ref, const uint32_t *ref_start,
                  const char *const *headers, const uint64_t *header_len);

#ifdef __cplusplus
}
#endif
#endif /* HW1_HOST_H */
