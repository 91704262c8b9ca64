/* vc_verkle.h -- verkle-tree commitments over libvkzg.so.
 *
 * Mirrors /root/reference/verkle-tree/src: VerkleTree<N, u8, VC, U256> (lib.rs:85-138) and
 * Node (node.rs:35-277): Internal / Extension nodes, insert (node.rs:133-204), get
 * (node.rs:74-95, lib.rs:119-125), path_to_stem (node.rs:97-120) and gen_commitment
 * (node.rs:205-277). Keys are N units of u8 (the reference tests' KEY_DATA_TYPE); values are
 * 32-byte U256 split into two Fr halves (low = bytes 0..16, high = bytes 16..32, LE, as the
 * tests' SplittableValue, lib.rs:186-194).
 *
 * The commitment is computed level by level: every dirty extension node of the tree goes
 * into one batched width-N commit (c1, c2), one batched to_data_item and one batched
 * width-4 commit; then every dirty internal node of one depth goes into one batched
 * width-256 commit, deepest level first -- instead of the reference's one recursive commit
 * per node. Rows are sparse: an internal node has a few non-zero children of 256, so only
 * non-zeros are expanded into table points. The commitment scheme is whatever `table` holds:
 * the KZG Lagrange SRS (vc_kzg_setup) or an IPA CRS (vc_bases_upload), BN254 G1.
 *
 * Device residency (vc_verkle_commitment, one context): every node's commitment, identity flag
 * and to_data_item live in a device mirror between calls (indexed by node id), so a level's
 * rows read their children's items there and nothing returns to the host but the root; the
 * host sends only the extension leaf values and each level's (column, child id) lists. An
 * updated internal node whose last commitment is in the mirror is recommitted as a delta row,
 * C_old + sum over the slots changed since of (item(new child) - item(old child)) L_slot (the
 * slots are logged at insert time) -- the same group element as its full row. A call that
 * fails leaves every dirty node to be recommitted in full by the next one. VKZG_VERKLE_DEV=0
 * (read per call) takes the host-built path the sharded / group commitments use.
 *
 * Reference quirks kept: the extension commit width is the key length
 * N, not 256; the stem keeps the key's last unit; internal nodes commit at width 256;
 * a key that differs from an existing extension's stem only in the last unit makes the
 * reference panic ("Traversed to extension node with differing stem") -- here insert
 * returns VC_E_INVALID and leaves the tree unchanged. */
#ifndef VC_VERKLE_H
#define VC_VERKLE_H
#include <stddef.h>
#include <stdint.h>

#include "vc_msm.h"
#include "vc_scheme.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vc_verkle vc_verkle;

/* VerkleTree::new (lib.rs:104-110); key_len = N (2..32 units of u8) */
vc_verkle* vc_verkle_new(int key_len);
void vc_verkle_free(vc_verkle* t);
/* insert_single (lib.rs:112-116): key = N bytes, value = 32 bytes */
int vc_verkle_insert(vc_verkle* t, const uint8_t* key, const uint8_t* value32);
/* get_single (lib.rs:118-125): *found = 0 when absent */
int vc_verkle_get(const vc_verkle* t, const uint8_t* key, uint8_t* value32, int* found);
/* path_to_stem (lib.rs:131-137): up to max_len entries of (prefix length, unit); *len set;
 * VC_E_INVALID for the reference's InvalidPath */
int vc_verkle_path(const vc_verkle* t, const uint8_t* key, size_t max_len, uint8_t* units, size_t* len);
/* commitment (lib.rs:127-129): root commitment, canonical affine BN254 G1 (x, y: 4 u64 each) */
int vc_verkle_commitment(vc_ctx* ctx, int table, vc_verkle* t, uint64_t* out_xy, uint8_t* out_inf);
/* diagnostics: per node id (up to max) its type (0 internal, 1 extension), level and committed
 * to_data_item (4 u64, canonical); *n = the node count */
int vc_verkle_debug_nodes(vc_verkle* t, size_t max, uint8_t* type, int32_t* level, uint64_t* items, size_t* n);
/* diagnostics (no GPU): the device path's extension host stage -- c1 / c2 rows of every
 * extension node built and merged into one buffer -- run `reps` times; *us = the median (us) */
int vc_verkle_debug_ext_stage(vc_verkle* t, int reps, double* us);
/* node counts (diagnostics): internal, extension, dirty */
int vc_verkle_stats(const vc_verkle* t, size_t* internal, size_t* extension, size_t* dirty);

/* ---------------------------------------------------------------- tree proofs
 * A proof shows that n keys, all present in the tree, map to their values under the root
 * commitment: one multiproof (vc_scheme.h, multiproof.rs) over the openings on the keys' paths.
 * The reference declares this (verkle-tree/src/lib.rs:140-152, an empty impl block) and stops.
 * Proofs of absence are out of scope: a key vc_verkle_get does not find is VC_E_INVALID.
 *
 * Path of key K (N units): the nodes vc_verkle_get / vc_verkle_path walk. d = the number of
 * internal nodes on it, the root I_0 included (1 <= d <= N - 1); I_{j+1} is the child of I_j at
 * position K[j] (also below the reference's level-skipping splits: position j is always indexed
 * with K[j]); the child of I_{d-1} at K[d-1] is the extension E whose stem is K, the whole key
 * (lib.rs:61-67). u = K[N-1], half = (u < N / 2) ? 1 : 2, C_half = the extension's c1 or c2
 * commitment (node.rs:216-244), (lo, hi) = the value's bytes 0..16 and 16..32 as LE integers.
 *
 * Queries (commitment, z, y) of K, in this order, all over the domain of size 256 (a row of width
 * 4 or N is the same group element as its zero-padded width-256 row, so it is opened there):
 *   1. for j = 0 .. d-1:  C(I_j),  z = K[j],            y = to_data_item(C(next)), next = I_{j+1}, or E
 *                                                           for j = d-1
 *   2.                    C(E),    z = 0,               y = 1
 *   3.                    C(E),    z = 1,               y = from_le_bytes_mod_order(K) (node.rs:248)
 *   4.                    C(E),    z = 1 + half,        y = to_data_item(C_half)
 *   5.                    C_half,  z = (2 u) % N,       y = lo
 *   6.                    C_half,  z = (2 u + 1) % N,   y = hi
 * The query list is the keys' queries in the caller's key order, a (node, z) pair that was emitted
 * before left out (a repeated key adds nothing); that order is the multiproof transcript's. Nodes
 * are told apart by where they sit: an internal node at position j by the units K[0..j), an
 * extension by its full key, a C_half by (full key, half). The `% N` folding of node.rs:231-232
 * can make two leaves of one extension share a slot; a key whose row no longer holds (lo, hi) at
 * its two slots cannot be proven (VC_E_INVALID).
 *
 * The proof: depth[i] = d of key i; the distinct commitments other than the root in
 * first-occurrence order of that walk (per key: the internal nodes at positions 1 .. d-1, then
 * C(E), then C_half); the multiproof's D; and the inner proof at the multiproof's t -- an IPA proof
 * (scheme 0) or the KZG proof point and y (scheme 1). All arrays are the caller's. */
typedef struct {
    size_t n_keys;      /* in: the keys proven (the length of depth) */
    uint8_t* depth;     /* n_keys */
    size_t n_com;       /* prove: in = the capacity of com_xy / com_inf, out = the commitments written */
    uint64_t* com_xy;   /* n_com x 8 u64, canonical affine */
    uint8_t* com_inf;   /* n_com identity flags */
    uint64_t d_xy[8];
    uint8_t d_inf;
    vc_ipa_proof ipa;   /* scheme 0: rounds = 8 with its four arrays */
    uint64_t kzg_proof_xy[8];  /* scheme 1 */
    uint8_t kzg_proof_inf;
    uint64_t kzg_y[4];
} vc_verkle_proof;
/* host only, no GPU: the commitments (n_com) and queries a proof of these n keys (n x N bytes)
 * holds; VC_E_INVALID for an absent or unprovable key */
int vc_verkle_proof_size(const vc_verkle* t, const uint8_t* keys, size_t n, size_t* n_com, size_t* n_queries);
/* scheme 0: IPA, `table` holds the 257 points g[0..256], q; scheme 1: KZG, `table` is the
 * size-256 Lagrange SRS; any other scheme or table size is VC_E_TABLE. It must be the table the tree is
 * committed with. If any node is dirty the tree is first committed as vc_verkle_commitment does
 * with this context and table. root_xy / root_inf: the root the proof is against. Nothing is
 * written when a key is absent or unprovable. The field phase reads the opened rows' non-zeros
 * where they are (the children's items in the device mirror) instead of building Q x 256 rows. */
int vc_verkle_prove(vc_ctx* ctx, int scheme, int table, vc_verkle* t, const uint8_t* keys, size_t n,
                    uint64_t* root_xy, uint8_t* root_inf, vc_verkle_proof* out);
/* needs no tree: rebuilds the query list from (root, keys, values32, proof->depth, the proof's
 * commitments) as above -- y of queries 1 and 4 is to_data_item of the proof's commitments
 * (vc_to_data_item_batch) -- and runs vc_multiproof_verify_ipa (scheme 0, `table` as for prove) or
 * vc_multiproof_verify_kzg (scheme 1, vk of the size-256 domain; `table` unused). *result = 1
 * valid, 0 invalid. Verdict 0 with VC_OK for: a depth outside 1..N-1; two keys that put different
 * node kinds, or two different extensions, at one position; a (node, z) pair the keys give two
 * different y; a commitment count that does not match the walk; a malformed point; an inner
 * verification that fails. VC_E_INVALID only for null or inconsistent arguments (n_keys != n). */
int vc_verkle_verify(vc_ctx* ctx, int scheme, int table, const vc_kzg_vk* vk, int key_len, const uint64_t* root_xy,
                     uint8_t root_inf, const uint8_t* keys, const uint8_t* values32, size_t n,
                     const vc_verkle_proof* proof, int* result);
/* diagnostics (nothing in the product path calls it): the prover's query list -- commitments
 * (max_q x 8, max_q), z (max_q), y (max_q x 4) -- and, if rows is not NULL, its zero-padded dense
 * rows (max_q x 256 x 4 u64) on the host, built from the tree's host arrays (the device mirror is
 * read back first); *Q = the number of queries (VC_E_RANGE if above max_q). Commits a dirty tree
 * first, as vc_verkle_prove. */
int vc_verkle_proof_queries(vc_ctx* ctx, int table, vc_verkle* t, const uint8_t* keys, size_t n, size_t max_q,
                            uint64_t* com_xy, uint8_t* com_inf, uint64_t* z, uint64_t* y, uint64_t* rows, size_t* Q);

#ifdef __cplusplus
}
#endif
#endif /* VC_VERKLE_H */
