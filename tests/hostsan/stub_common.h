// stub_common.h — fault injection and jitter shared by hip_stub.cpp and ks_stub.cpp.
//
// TEST INFRASTRUCTURE ONLY (tests/hostsan/): a CPU stand-in for the part of the ABI the host layer calls, so that
// ks_ingest.cpp, ks_host.cpp and ks_input.cpp run under the host sanitizers.  Nothing under kmerseek_amd/ or include/
// may include or link any file of this directory.
#ifndef HOSTSAN_STUB_COMMON_H
#define HOSTSAN_STUB_COMMON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The n-th call (1-based, counted from now) of the stubbed function `fn` fails with `status` (a hipError_t for the
 * runtime calls, a ks_status for the ks_* ones).  Several faults may be armed; stub_reset disarms all and zeroes the counts. */
void stub_fail_nth(const char *fn, int n, int status);
/* Every stubbed call first sleeps a seeded pseudo-random 0..max_us microseconds (max_us = 0: no sleep). */
void stub_jitter(uint64_t seed, unsigned max_us);
/* Calls of `fn` since the last stub_reset (the test programs size "a middle call" and "the last call" from a clean run). */
int stub_call_count(const char *fn);
void stub_reset(void);
/* Bytes the stubbed runtime has handed out and not got back: 0 after a clean teardown. */
uint64_t stub_live_bytes(void);

/* While on, ks_sketch_batch_device appends the residues and the record lengths it is handed (what the packer made of the
 * file) to a buffer the test program reads back; stub_capture(0) stops, stub_capture(1) also clears. */
void stub_capture(int on);
const uint8_t *stub_captured_residues(uint64_t *n);
const uint64_t *stub_captured_lengths(uint64_t *n);

/* for the stubs themselves: jitter, count the call, return the armed status or 0 */
int stub_enter(const char *fn);

#ifdef __cplusplus
}
#endif
#endif
