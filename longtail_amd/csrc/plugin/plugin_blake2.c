/* plugin_blake2.c -- Longtail_HashAPI 'blk2' (BLAKE2s, 64-bit) on the GPU: the object of plugin_hash.c over the lthip_blake2s_* calls.
 *
 * Mirrors lib/blake2/longtail_blake2.c of the reference: Longtail_CreateHipBlake2HashAPI <-> Longtail_CreateBlake2HashAPI,
 * GetIdentifier -> 'blk2' 0x626c6b32, BeginContext / Hash / EndContext / HashBuffer as the BLAKE3 object's.
 *
 * Paired with the HIP chunker.  A published window carries BLAKE3 digests.  Its BLAKE2 table is filled lazily: the first HashBuffer of
 * one of its chunks hashes ALL of the window's chunks with one lthip_blake2s_ranges call, and every later HashBuffer of the window is
 * a table read (ltp_window_table_lookup, plugin_hash.c).  Anything else is hashed on the GPU by itself.
 */
#include "plugin_common.h"

#define LONGTAIL_HIP_BLAKE2_ID ((((uint32_t)'b') << 24) + (((uint32_t)'l') << 16) + (((uint32_t)'k') << 8) + ((uint32_t)'2'))

/* plugin_hash.c collects stream batches of LTHIP_B3_STREAM_BATCH bytes for every kind */
#if LTHIP_B3_STREAM_BATCH != LTHIP_B2S_STREAM_BATCH
#error "the BLAKE3 and BLAKE2s stream batches differ"
#endif

static const struct ltp_hash_kind g_blake2 = {LONGTAIL_HIP_BLAKE2_ID, lthip_blake2s_one, lthip_blake2s_ranges, lthip_b2s_stream_batch,
                                              lthip_b2s_stream_final, LTHIP_B2S_STREAM_STATE_BYTES, 0, ltp_window_table_lookup};

struct Longtail_HashAPI* Longtail_CreateHipBlake2HashAPI(void) { return ltp_create_hash_api(&g_blake2); }
