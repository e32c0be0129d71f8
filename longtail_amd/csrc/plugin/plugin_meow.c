/* plugin_meow.c -- Longtail_HashAPI 'meow' (Meow hash v0.5, 64-bit) on the GPU: the object of plugin_hash.c over the lthip_meow_*
 * calls.
 *
 * Mirrors lib/meowhash/longtail_meowhash.c of the reference: Longtail_CreateHipMeowHashAPI <-> Longtail_CreateMeowHashAPI,
 * GetIdentifier -> 'meow' 0x6d656f77, BeginContext / Hash / EndContext / HashBuffer as the BLAKE3 object's; the digest is
 * MeowU64From(MeowEnd(state), 0) after MeowBegin(MeowDefaultSeed) and MeowAbsorb.
 *
 * Paired with the HIP chunker, a window's Meow digests are filled for all of its chunks by the first HashBuffer of one of them (one
 * lthip_meow_ranges call, ltp_window_table_lookup in plugin_hash.c).  The window holds one such table, tagged with the kind that
 * filled it: a BLAKE2 object's look-up of the same window fills it again with BLAKE2 digests, and neither object is handed the
 * other's.  Anything else is hashed on the GPU by itself.
 */
#include "plugin_common.h"

#define LONGTAIL_HIP_MEOW_ID ((((uint32_t)'m') << 24) + (((uint32_t)'e') << 16) + (((uint32_t)'o') << 8) + ((uint32_t)'w'))

/* plugin_hash.c collects stream batches of LTHIP_B3_STREAM_BATCH bytes for every kind; a Meow batch is whole 256-byte blocks */
#if LTHIP_B3_STREAM_BATCH != LTHIP_MEOW_STREAM_BATCH || (LTHIP_MEOW_STREAM_BATCH % 256) != 0
#error "the Meow stream batch must be the BLAKE3 batch, a multiple of 256 bytes"
#endif

static const struct ltp_hash_kind g_meow = {LONGTAIL_HIP_MEOW_ID, lthip_meow_one, lthip_meow_ranges, lthip_meow_stream_batch,
                                            lthip_meow_stream_final, LTHIP_MEOW_STREAM_STATE_BYTES, 0, ltp_window_table_lookup};

struct Longtail_HashAPI* Longtail_CreateHipMeowHashAPI(void) { return ltp_create_hash_api(&g_meow); }
