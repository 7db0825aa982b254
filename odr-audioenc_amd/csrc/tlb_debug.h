/* tlb_debug.h -- TEST BUILDS ONLY.  Fault injection for the error paths no healthy GPU takes: compiled into the library only with
 * -DTLB_FAULT_INJECT (csrc/Makefile target `fault`: odr-audioenc_amd/libtoolame_dab_hip_fi.so, the product's kernel objects + the host
 * files rebuilt with the flag).  The product library has none of this: no symbol, no branch (tests/test_abi_symbols.py checks the list).
 * An armed launch fails exactly as a failing device call inside it would: tlb_launch returns TLB_ERR_HIP after its guard has marked
 * the batch broken. */
#pragma once
#include "../../include/toolame_batch.h"
#ifdef __cplusplus
extern "C" {
#endif
int tlb_debug_fail_next(tlb_batch *b, int nth);                    /* the nth launch of this batch from now fails (1 = the next; 0 disarms) */
int tlb_debug_tick_fail_next(tlb_tick *t, int nth);                /* ... the nth submit of this tick object, in its LAST group: the groups before it have been queued */
/* The nth submit from now (1 = the next; 0 disarms) XORs byte `byte` of that stream's slot in the tick's device frame buffer with xor_mask, after the
 * encode and before the egress and the confidence monitor: the caller receives the damaged frame and the monitor sees the same bytes.  A
 * host-queued one-byte copy out and back in; it does not fault the device. */
int tlb_debug_tick_damage_next(tlb_tick *t, int stream, int byte, int xor_mask, int nth);
/* From the nth submit from now ON (1 = the next; 0 disarms; tlb_tick_finish included) the slots of streams a and b of one group are exchanged in
 * the tick's device frame buffer, lengths too, after the encode and before the egress and the monitors, tick after tick: valid frames that
 * carry the other stream's programme.  The caller receives the exchanged frames.  Device-to-device copies on the tick's own stream. */
int tlb_debug_tick_cross_from(tlb_tick *t, int a, int b, int nth);
int tlb_debug_node_fail_next(tlb_node *nd, int shard, int nth);    /* ... of one shard of a node */
/* A stalled shard for the node's tick deadline: the nth wait job of that shard from now (1 = the next; 0 disarms), AFTER its
 * tlb_tick_wait has returned with the tick complete, sleeps `ms` on the shard's HOST thread and then returns `rc` (0: the tick's results
 * stand; non-zero: as a failing call would).  The device stays idle and healthy: no kernel spins, no event is left incomplete. */
int tlb_debug_node_stall_next(tlb_node *nd, int shard, int nth, int ms, int rc);
/* The nth allocation through the library's memory owner (csrc/tlb_mem.h: device or pinned) from now, PROCESS-WIDE, is refused without a call
 * to the runtime (1 = the next; 0 disarms): the creation, first-use and opt-in paths then fail as they would when memory runs out.  The
 * counter is atomic (node shards allocate on their own threads).  Nothing is launched and the device is not touched. */
int tlb_debug_alloc_fail_next(int nth);
/* The probe (csrc/mp2_probe.h, csrc/toolame_probe.hip): ONE form of csrc/tl_libm.h's device half (form: TLP_LOG_PN ...; table: 0 = the global
 * table, 1 = its LDS copy, log family only) over n arguments a[i] (and b[i] where the form takes two; else b may be NULL), results to r0[i] (and
 * r1[i] where it returns two; else r1 may be NULL) -- resp. ONE cross-lane primitive of csrc/mp2_wave.h (prim: TLP_WAVE_MIN_U64 ...) over nwaves
 * cases of 64 64-bit words (layout at the enum).  HOST pointers: device buffers through the library's memory owner, one launch on the current
 * device, waited for, copied out.  TLB_ERR_ARG for an unknown form / primitive, n <= 0, a missing pointer and for ANY argument outside the
 * form's stated domain (tlp_in_domain): checked on the host before anything is queued, so nothing out of domain reaches the device. */
int tlb_debug_probe_libm(int form, int table, long n, const double *a, const double *b, double *r0, double *r1);
int tlb_debug_probe_wave(int prim, int nwaves, const void *in, const void *in2, void *out);
/* The third family (csrc/mp2_probe_stage.h): ONE group of the stage helpers of csrc/mp2_dbsum.h (form: TLS_ADD_DB ...) over n lane-arguments or n cases of a
 * wave; the arrays and their layouts are stated at the enum, an array a form does not have may be NULL.  HOST pointers, the library's memory owner, one
 * launch, waited for, copied out, like the two above.  TLB_ERR_ARG for an unknown form, n <= 0, a missing pointer and for ANY argument or case outside
 * the form's stated domain (tls_in_domain) -- checked on the host before anything is queued: the helpers make LDS indexes from counts, rows and lengths.
 * The last form, TLS_ALLOC, is one layer up: the bit allocation of csrc/mp2_alloc.h alone (tl_allocate, or tl_allocate_pair for two mono streams), one
 * wave per case, from an allocation table, nch, jsbound, the frame's bits and per lane an SMR and a scfsi; it returns ba of all 64 lanes and the bits left. */
int tlb_debug_probe_stage(int form, long n, const void *in0, const void *in1, const void *in2, void *out0, void *out1);
#ifdef __cplusplus
}
#endif
