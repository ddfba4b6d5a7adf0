/*
 * rg_aead.h -- C ABI of the MI355X (gfx950) WireGuard transport-data AEAD
 * engine.  Drop-in boundary for the reference's hot path:
 *
 *   trait CryptoPrimatives (rustyguard-crypto/src/prim.rs:74-111)
 *     fn chacha20poly1305_enc(key, nonce, aad, payload, tag)      prim.rs:82-88
 *     fn chacha20poly1305_dec(key, nonce, aad, payload, tag)      prim.rs:89-95
 *     fn xchacha20poly1305_enc / _dec (24-byte nonce)            prim.rs:97-110
 *   impl for Core (graviola 0.2.0 underneath)                     prim.rs:179-201
 *   EncryptionKey::encrypt  (counter++, nonce, seal)              prim.rs:376-399
 *   DecryptionKey::decrypt  (replay gate, open, mark_seen)        prim.rs:401-437
 *   AntiReplay::{would_accept, mark_seen}                         rustyguard-utils/src/anti_replay.rs:25-64
 *   PeerState::force_encrypt + EncryptedMetadata::frame_in_place  rustyguard-core/src/lib.rs:267-297, :450-470
 *   Sessions::recv_message / decrypt_packet                       rustyguard-core/src/lib.rs:605-681
 *
 * The per-packet trait shape would pay a PCIe round trip per packet, so the
 * primary entry points are BATCHED.  All calls are plain C: no exceptions or
 * panics cross the ABI, every function returns RG_OK (0) or a negative
 * rg_status; per-packet outcomes go to a caller-owned status array.
 *
 * Buffer contract (same for device and host variants)
 * ---------------------------------------------------
 *  buf            one byte arena holding wire frames; frame i starts at
 *                 desc[i].offset, which must be 16-byte aligned (mirrors
 *                 AlignedPacket, rustyguard-tun/src/lib.rs:21-24, and the
 *                 alignment check of rustyguard-core/src/lib.rs:613-615).
 *  frame layout   [DataHeader 16 B][payload P B][Tag 16 B]   (W = P + 32)
 *                 DataHeader = {u32 type=4, u32 receiver, u64 counter}, LE
 *                 (rustyguard-types/src/lib.rs:152-179).
 *  seal           desc[i].len = P (payload bytes, P % 16 == 0: the
 *                 assert of rustyguard-core/src/lib.rs:273-277).  The
 *                 payload is encrypted in place, the header (if receivers
 *                 != NULL) and the tag are written into the frame
 *                 (frame_in_place, lib.rs:463-469).  nonce =
 *                 00000000 || le64(counters[i]) (prim.rs:32-36), AAD empty.
 *  open           desc[i].len = W (whole frame).  The counter is read from
 *                 the header, the tag from the last 16 bytes; on success the
 *                 payload is decrypted in place.  On any failure the frame is
 *                 left byte-for-byte unchanged.
 *  keys           key table, nkeys rows of 32 bytes; desc[i].key_idx picks
 *                 the row (one row per session direction).
 *  frames         the frames of one call must not overlap (each is its own
 *                 datagram, as in the reference); they may come in any order.
 */
#ifndef RG_AEAD_H
#define RG_AEAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_ABI_VERSION 6

typedef struct rg_ctx rg_ctx;

/* 16-byte packet descriptor; device copies must be 16-byte aligned. */
typedef struct rg_pkt_desc {
    uint64_t offset;  /* frame offset in buf, multiple of 16 */
    uint32_t len;     /* seal: payload length P; open: frame length W */
    uint32_t key_idx; /* key-table row; RG_KEY_SKIP = leave packet untouched */
} rg_pkt_desc;

#define RG_KEY_SKIP 0xFFFFFFFFu

/* call status */
typedef enum rg_status {
    RG_OK = 0,
    RG_EINVAL = -1,  /* bad argument (null pointer, n too large, ...) */
    RG_EDEVICE = -2, /* HIP runtime error; rg_last_error() has the text */
    RG_ENOMEM = -3,
    RG_ENOTFOUND = -4,
    RG_EFULL = -5,
} rg_status;

/* per-packet status (uint8_t), numbering shared with the CPU oracle.
 * Maps onto rustyguard_core::Error (rustyguard-core/src/lib.rs:416-423). */
enum rg_pkt_status {
    RG_PKT_OK = 0,
    RG_PKT_DECRYPT_ERR = 1, /* Error::DecryptionError: tag mismatch / < 16 B after header */
    RG_PKT_INVALID = 2,     /* Error::InvalidMessage: W % 16 != 0, W < 16, message type
                               not 1-4 (lib.rs:627), bad seal desc */
    RG_PKT_REJECTED = 3,    /* Error::Rejected: replayed/too old counter, no session,
                               REJECT_AFTER_MESSAGES reached, or RG_KEY_SKIP */
    RG_PKT_UNALIGNED = 4,   /* Error::Unaligned: frame not 16-byte aligned */
    RG_PKT_NOT_DATA = 5,    /* type 1, 2 or 3 (handshake init/resp, cookie): route to the
                               handshake path (lib.rs:622-624) */
    RG_PKT_PENDING = 6,     /* no verdict: the packet was never finished (the call failed, a device
                               error, or a batch still in flight).  Never an accept. */
    RG_PKT_COOKIE = 7,      /* rg_cookie_reply_batch_dev: mac1 valid, mac2 missing or wrong while overloaded;
                               a cookie reply was written for this message */
    RG_PKT_KEYEXCHANGE = 8, /* Error::KeyExchangeError: an X25519 result was all zero (rg_x25519_batch_dev and
                               the handshake calls) */
    RG_PKT_UNROUTABLE = 9,  /* cryptokey routing (rg_route_batch_dev, rg_route_check_batch_dev): the inner address
                               matches no allowed prefix, or on receive a prefix of another peer */
    RG_PKT_FULL = 10,       /* rg_session_install_batch_dev: the session table has no free row left;
                               rg_demux_batch_dev: the message's list has no row left */
};

/* Statuses fail closed.  A packet reads RG_PKT_OK only after the kernel that processed it wrote that
 * verdict: every launch that hands packets from one workgroup to another (the planned pipelined kernel,
 * the tile kernels) is preceded, on the same stream, by a preset pass that sets the batch's statuses to
 * RG_PKT_PENDING and clears the planner's control words; the launches without a hand-off (the pipelined
 * kernel in array order, the flattened kernel) deal every packet to a lane by its index alone, and that
 * lane writes its status.  The host-memory calls (rg_*_batch_host*, rg_send_batch, rg_recv_batch*) check
 * after the device work that no status is still RG_PKT_PENDING (RG_EDEVICE otherwise), and every host-memory
 * call that returns an error leaves all n statuses RG_PKT_PENDING: no replay window or endpoint moves on
 * a failed batch.  rg_recv_batch_dev_finish runs the replay pass only over RG_PKT_OK / RG_PKT_DECRYPT_ERR
 * verdicts and returns RG_EDEVICE when any packet is still pending. */

/* ---------------------------------------------------------------- context */

int rg_abi_version(void);
/* Create a context bound to HIP device `device` (one per process/GPU).  Every call on a context works on
 * its device and leaves the caller's current HIP device as it found it.  Key material the context keeps
 * in device memory (the host calls' key table, the MAC key states, the per-message arena) is zeroed
 * before its memory is reused or freed, in stream order: behind the launches that read it, without
 * waiting for the device or for other streams (prim.rs:227-231 zeroizes keys on drop).  A call that would
 * have to regrow such a buffer while its stream is being captured into a graph fails with RG_EDEVICE.  A
 * block that a captured launch reads is never freed under the graph: a later regrow takes a new block and
 * keeps the captured one allocated until rg_destroy (rg_sessions_destroy for a session table's rows),
 * which zeroes and frees it; such a graph must not be replayed after that.  rg_create refuses (RG_EINVAL)
 * to run under ROC_SYSTEM_SCOPE_SIGNAL=0: agent-scope completion signals hung the host pipeline's waits in
 * round 5 (profiles/r5_e2e_rtenv.txt). */
int rg_create(int device, rg_ctx **out);
void rg_destroy(rg_ctx *ctx);
/* Text of the last error on this thread ("" if none). */
const char *rg_last_error(void);

/* --------------------------------------- device-resident batch (async) */
/* Every pointer is device memory; work is enqueued on `stream`
 * (hipStream_t, NULL = legacy default stream) and the call returns without
 * synchronising.  status is required (ABI 6: it is how a caller knows a packet
 * was sealed; RG_PKT_OK is written only by the lane that sealed it), receivers /
 * counters_out may be NULL.  The kernels bounds-check every descriptor against
 * buf_len and never touch memory outside [buf, buf + buf_len).  Calls on one
 * context are ordered on one stream (they share the planner buffers and the tile
 * kernel's work pool, see rg_set_plan); use a context per concurrent stream.  A
 * call on another stream while this context's last batch is still in flight on
 * its stream fails with RG_EINVAL and enqueues nothing (the check needs no
 * wait: an event query).  Launches captured into a graph are not tracked: a
 * caller that replays such a graph orders the replays against the context's
 * other calls itself (same stream, or events). */
int rg_seal_batch_dev(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                      const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *buf, size_t buf_len,
                      uint8_t *status, void *stream);
int rg_open_batch_dev(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys, const rg_pkt_desc *desc, size_t n,
                      uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out, void *stream);

/* ------------------------------------ device-side receiver resolution */
/* The receiver-index -> session map of Sessions::decrypt_packet
 * (rustyguard-core/src/lib.rs:646-650, `peers_by_session`) as an
 * open-addressing table: slot = (receiver * 0x9E3779B1) >> (32 - log2 cap),
 * linear probing, key_idx == RG_KEY_SKIP marks an empty slot.  Built on the
 * host (cap a power of two >= 2 n; receivers unique), used on the device. */
typedef struct rg_rx_entry {
    uint32_t receiver;
    uint32_t key_idx;
} rg_rx_entry;
int rg_rx_table_build(const uint32_t *receivers, const uint32_t *key_idx, size_t n, rg_rx_entry *table,
                      uint32_t cap);
/* host lookup: key index, or -1 when the receiver has no session */
int64_t rg_rx_table_find(const rg_rx_entry *table, uint32_t cap, uint32_t receiver);
/* rg_open_batch_dev for frames straight off the wire: desc[i].key_idx is
 * ignored; each frame's session comes from its header's receiver index through
 * rx_table (device memory), in the reference's check order -- alignment,
 * message type and 16-byte framing first (their statuses as rg_open_batch_dev),
 * then an unknown receiver is RG_PKT_REJECTED (`Error::Rejected`, lib.rs:
 * 647-650), then the AEAD.  key_idx_out (device, may be NULL) receives the
 * resolved key index (RG_KEY_SKIP when none) for the host's anti-replay pass. */
int rg_open_batch_dev_rx(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys, const rg_rx_entry *rx_table,
                         uint32_t rx_cap, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                         uint8_t *status, uint64_t *counters_out, uint32_t *key_idx_out, void *stream);

/* ----------------------------------------- handshake MAC checks (batch) */
/* HasMac::verify_mac1 / verify_mac2 (rustyguard-crypto/src/lib.rs:114-209)
 * for n handshake messages (desc: offset, len = whole message incl. both
 * macs): mac1 = BLAKE2s-128(keys[k], msg[..len-32]) against msg[len-32..
 * len-16] (which = 1, 32-byte mac1 keys), mac2 = BLAKE2s-128(cookie,
 * msg[..len-16]) against msg[len-16..] (which = 2, 16-byte cookies).
 * status: RG_PKT_OK, RG_PKT_REJECTED (mismatch: CryptoError::Rejected),
 * RG_PKT_UNALIGNED, RG_PKT_INVALID (len < 32 or outside buf).  key_idx
 * RG_KEY_SCAN tries every key and reports the first match in key_idx_out
 * (wg-proxy's peer scan, wg-proxy/src/main.rs:217-229).  Device pointers. */
#define RG_KEY_SCAN 0xFFFFFFFEu
int rg_mac_verify_batch_dev(rg_ctx *ctx, const uint8_t *keys, uint32_t key_len, uint32_t nkeys, int which,
                            const rg_pkt_desc *desc, size_t n, const uint8_t *buf, size_t buf_len, uint8_t *status,
                            uint32_t *key_idx_out, void *stream);

/* ------------------------------- under-load handshake filter (batch) */
/* HasMac::verify with overload = true (rustyguard-crypto/src/lib.rs:114-140) followed by
 * Sessions::write_cookie_message (rustyguard-core/src/lib.rs:517-540) for n handshake messages in one
 * launch: mac1 under the server's mac1 key, then -- while overloaded -- mac2 under the message's own
 * cookie = BLAKE2s-128(secret, source address) (CookieState::new_cookie, lib.rs:95-104), and for every
 * message whose mac2 fails a sealed 64-byte CookieMessage.  All pointers are device memory; the call
 * enqueues on `stream` and returns without waiting, like rg_mac_verify_batch_dev.  buf is never written.
 * The call keeps nothing in the context: the two key-only BLAKE2s states are recomputed by every
 * workgroup and live in LDS, so calls on one context may run on any streams.
 *
 * desc[i]: offset, len = whole message.  Per message, in this order:
 *   offset % 16 != 0                                   RG_PKT_UNALIGNED
 *   frame outside [buf, buf + buf_len), or len neither
 *   148 (initiation) nor 92 (response)                 RG_PKT_INVALID
 *   key_idx == RG_KEY_SKIP                             RG_PKT_REJECTED, nothing read (any other key_idx
 *                                                      is ignored)
 *   type word != 1 for len 148 / != 2 for len 92       RG_PKT_INVALID (Error::InvalidMessage)
 *   mac1 = BLAKE2s-128(mac1_key, msg[..len-32]) differs
 *   from msg[len-32..len-16]                           RG_PKT_REJECTED, whatever mac2 says
 *   overload && overload[i] == 0                       RG_PKT_OK
 *   mac2 = BLAKE2s-128(cookie, msg[..len-16]) equals
 *   msg[len-16..]                                      RG_PKT_OK: on to the handshake
 *   otherwise                                          RG_PKT_COOKIE and replies[i] =
 *       le32(3) || msg.sender (bytes 4..8) || nonces[i] || ct(16) || tag(16), with (ct, tag) =
 *       XChaCha20-Poly1305(cookie_key, nonces[i], aad = the message's mac1 field, pt = cookie)
 *       (encrypt_cookie, rustyguard-crypto/src/lib.rs:61-70).
 * Reply rows of messages with any other status are not touched.  Statuses fail closed: the lane that
 * judged a message writes its status, after its reply stores.
 *
 * Randomness: the library has no RNG.  nonces[i] must be 24 fresh bytes of the caller's CSPRNG for
 * every message of every call (the reference draws them from its session RNG, rustyguard-core/src/
 * lib.rs:529-530); their uniqueness and unpredictability are the caller's responsibility.  secret is
 * CookieState.key, which the caller also rotates (lib.rs:79-93).
 *
 * n == 0 returns RG_OK.  RG_EINVAL, nothing enqueued: a null pointer (overload may be NULL = all
 * overloaded), n > 2^32 - 1, keys or replies not 16-byte aligned, addrs or nonces not 8-byte aligned. */
typedef struct rg_cookie_keys {      /* device memory, 16-byte aligned, 96 bytes */
    uint8_t mac1_key[32];            /* mac1_key(own static public key), lib.rs:72-74 */
    uint8_t cookie_key[32];          /* cookie_key(own static public key), lib.rs:75-77: the XChaCha key */
    uint8_t secret[32];              /* CookieState.key, rotated by the caller (lib.rs:79-93) */
} rg_cookie_keys;

typedef struct rg_src_addr {         /* 24 bytes, 8-byte aligned; CookieState::new_cookie's encoding */
    uint8_t ip[16];                  /* IPv4: octets in ip[0..4], rest zero; IPv6: 16 octets */
    uint16_t port_le;                /* little-endian port */
    uint8_t pad[6];                  /* ignored: only the first 18 bytes are hashed */
} rg_src_addr;

int rg_cookie_reply_batch_dev(rg_ctx *ctx, const rg_cookie_keys *keys, const rg_pkt_desc *desc,
                              const rg_src_addr *addrs, const uint8_t *overload /* [n] or NULL = all overloaded */,
                              const uint8_t *nonces /* [n][24], caller's CSPRNG output */, size_t n,
                              const uint8_t *buf, size_t buf_len, uint8_t *replies /* [n][64], 16-byte aligned */,
                              uint8_t *status, void *stream);

/* ------------------------------ Noise IKpsk2 responder (batch, async) */
/* The step behind the filter above: Sessions::handle_handshake_init's cryptography (rustyguard-core/src/
 * handshake.rs:36-137) for every message the filter passed, without a host step per message.  All pointers
 * are device memory unless marked host; the calls enqueue on `stream` and return without waiting, keep
 * nothing in the context (so they may run on any stream and be captured into a graph) and never write buf.
 * n == 0 returns RG_OK; RG_EINVAL with nothing enqueued for a null required pointer, n > 2^32 - 1 or a
 * misaligned array (each call names its rule).
 *
 * rg_x25519_batch_dev is CryptoPrimatives::x25519 / x25519_pubkey (prim.rs:79-80, :159-177) for n rows, one
 * lane per row: out[i] = X25519(scalars[i], points[i]) as RFC 7748 §5 defines it (the scalar is clamped, bit
 * 255 of the point is masked, non-canonical points are accepted); points == NULL means the base point 9.
 * status[i] is RG_PKT_OK, or RG_PKT_KEYEXCHANGE when the result is all zero, in which case out[i] is 32 zero
 * bytes.  The all-zero result (RFC 7748 §6.1: a point of small order) is X25519's only failure and the only
 * one reported here; what else the reference's library (graviola, not available to this project) might
 * refuse in diffie_hellman is not known.  Constant time: no branch and no address depends on a scalar or a
 * result.  Rows must be 4-byte aligned. */
int rg_x25519_batch_dev(rg_ctx *ctx, const uint8_t *scalars /* [n][32] */,
                        const uint8_t *points /* [n][32], or NULL = the base point 9 */,
                        uint8_t *out /* [n][32] */, uint8_t *status /* [n] */, size_t n, void *stream);

typedef struct rg_hs_static {        /* 64 bytes, 16-byte aligned: StaticInitiatorConfig */
    uint8_t private_key[32];
    uint8_t public_key[32];          /* X25519(private_key, 9) */
} rg_hs_static;

typedef struct rg_hs_peer {          /* 96 bytes, 16-byte aligned rows: StaticPeerConfig */
    uint8_t public_key[32];
    uint8_t preshared_key[32];       /* zero when the peer has none */
    uint8_t mac1_key[32];            /* mac1_key(public_key), lib.rs:72-74 */
} rg_hs_peer;

typedef struct rg_hs_init_result {   /* 128 bytes, 16-byte aligned */
    uint8_t chain[32], hash[32];     /* HandshakeState after the initiation */
    uint8_t ephemeral[32];           /* the initiator's ephemeral public key (msg[8..40]) */
    uint8_t timestamp[12];           /* decrypted TAI64N */
    uint32_t peer;                   /* row of peers, RG_PEER_NONE unless status is RG_PKT_OK */
    uint32_t sender;                 /* msg[4..8] */
    uint8_t pad[12];
} rg_hs_init_result;

/* Config::get_peer_idx as an open-addressing table over peer rows, built on the host and read on the
 * device: table[slot] is a row of peers or 0xFFFFFFFF (empty), slot = (le32(public_key[0..4]) * 0x9E3779B1)
 * >> (32 - log2 cap), linear probing; cap a power of two >= 2 npeers.  A duplicate public key is RG_EINVAL.
 * The key comparison reads all 32 bytes with no early exit.  Host pointers.  rg_peer_table_find: the row of
 * pk, or -1. */
int rg_peer_table_build(const rg_hs_peer *peers, uint32_t npeers, uint32_t *table, uint32_t cap);
int64_t rg_peer_table_find(const rg_hs_peer *peers, const uint32_t *table, uint32_t cap, const uint8_t pk[32]);

/* rg_handshake_init_batch_dev: decrypt_handshake_init (rustyguard-crypto/src/lib.rs:346-384) and
 * Config::get_peer_idx for n messages.  desc[i]: offset, len = whole message.  Per message, in the
 * reference's order:
 *   offset % 16 != 0                                   RG_PKT_UNALIGNED
 *   frame outside [buf, buf + buf_len), or len != 148  RG_PKT_INVALID
 *   gate && gate[i] != RG_PKT_OK, or
 *   key_idx == RG_KEY_SKIP                             RG_PKT_REJECTED, message not read
 *   type word != 1                                     RG_PKT_INVALID
 *   X25519(own.private_key, ephemeral) all zero        RG_PKT_KEYEXCHANGE
 *   the encrypted static key's tag fails               RG_PKT_DECRYPT_ERR
 *   X25519(own.private_key, decrypted static) all zero RG_PKT_KEYEXCHANGE
 *   the encrypted timestamp's tag fails                RG_PKT_DECRYPT_ERR
 *   the static key is not in the table                 RG_PKT_REJECTED (after both fields opened, as
 *                                                      handshake.rs:75-82)
 *   otherwise                                          RG_PKT_OK, results[i] filled
 * gate lets rg_cookie_reply_batch_dev's status array feed this call on the same stream with no host step.
 * mac1 and mac2 are NOT checked here: run the filter first.  The row of every message whose status is not
 * RG_PKT_OK is written as 128 zero bytes with peer = RG_PEER_NONE, so no partial secret state is left
 * behind; a lane stores its status after its row.  The timestamp-replay check (peer.latest_ts,
 * handshake.rs:88-91) is an in-order pass per peer: rg_peer_ts_batch_dev (below) runs it on this call's
 * results and status on the same stream, before they go on to the response.
 * RG_EINVAL also for cap not a power of two; own, peers, desc and results must be 16-byte aligned,
 * peer_table 4-byte aligned. */
int rg_handshake_init_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers, uint32_t npeers,
                                const uint32_t *peer_table, uint32_t cap, const rg_pkt_desc *desc,
                                const uint8_t *gate /* [n] or NULL */, size_t n, const uint8_t *buf, size_t buf_len,
                                rg_hs_init_result *results, uint8_t *status, void *stream);

/* rg_handshake_resp_batch_dev: encrypt_handshake_resp (lib.rs:386-433) and HandshakeState::split(false)
 * (prim.rs:299-313) for n result rows.  Per row:
 *   gate && gate[i] != RG_PKT_OK      RG_PKT_REJECTED; nothing of the row is read or written
 *   results[i].peer >= npeers         RG_PKT_INVALID
 *   the ee or se secret all zero      RG_PKT_KEYEXCHANGE
 *   otherwise                         RG_PKT_OK: responses[i] = the 92-byte HandshakeResp
 *       le32(2) || session_ids[i] || results[i].sender || X25519(esk[i], 9) || tag(16) || mac1 || mac2
 *     (4 zero bytes behind it), mac1 under peers[peer].mac1_key over bytes 0..60, mac2 under cookies[i]
 *     over bytes 0..76 when cookies && has_cookie[i], else zero; transport_keys[i] = send key || receive
 *     key, the order rg_sessions_insert takes them (send = HKDF's second output, receive = the new chain).
 * On any failure the response row and the key row are zero.  results[i].chain and .hash are zeroed by every
 * row that was not gated off (HandshakeState::zeroize): a row is consumed once.
 * Randomness: the library has no RNG.  esk[i] must be 32 fresh bytes of the caller's CSPRNG for every row
 * of every call (EphemeralPrivateKey::generate, handshake.rs:98), never reused; session_ids[i] is the
 * caller's session index (allocate_session!).  peers, results, responses and transport_keys must be
 * 16-byte aligned, esk, session_ids and cookies 4-byte aligned; has_cookie is required with cookies. */
int rg_handshake_resp_batch_dev(rg_ctx *ctx, const rg_hs_peer *peers, uint32_t npeers, rg_hs_init_result *results,
                                const uint8_t *gate /* [n] or NULL */, const uint8_t *esk /* [n][32] */,
                                const uint32_t *session_ids /* [n] */, const uint8_t *cookies /* [n][16] or NULL */,
                                const uint8_t *has_cookie /* [n], required with cookies */, size_t n,
                                uint8_t *responses /* [n][96], 16-byte aligned, 92 bytes used */,
                                uint8_t *transport_keys /* [n][64]: send key || receive key */,
                                uint8_t *status, void *stream);

/* ------------------------------ Noise IKpsk2 initiator (batch, async) */
/* The other end of the handshake: the cryptography of Sessions::new_handshake (rustyguard-core/src/
 * handshake.rs:260-325) and of handle_handshake_resp (handshake.rs:140-230), so that a handshake can run between
 * two users of this library.  The conventions are the responder's: all pointers are device memory; the calls
 * enqueue on `stream` and return without waiting, keep nothing in the context (so they may run on any stream
 * and be captured into a graph); n == 0 returns RG_OK; RG_EINVAL with nothing enqueued for a null required
 * pointer, n > 2^32 - 1 or a misaligned array.  Struct rows, desc, messages and transport_keys must be 16-byte
 * aligned, word arrays (peer_idx, esk, timestamps, session_ids, cookies, pend_table, pend_idx_out, remote_out,
 * claim) 4-byte aligned.  Choosing session ids and the peer's endpoint stay with the caller; current_handshake and
 * the retry and expiry timers are the pending-handshake section's, and installing the finished sessions is
 * rg_session_install_finish_batch_dev's (both further down).
 *
 * Randomness and time: the library has no RNG and no clock.  esk[i] must be 32 fresh bytes of the caller's
 * CSPRNG for every row of every call (EphemeralPrivateKey::generate, handshake.rs:275), never reused;
 * session_ids[i] is the caller's session index (allocate_session!); timestamps[i] is the caller's TAI64N. */
typedef struct rg_hs_pending {       /* 128 bytes, 16-byte aligned: SessionHandshake + its session id */
    uint8_t chain[32], hash[32];     /* HandshakeState after the initiation */
    uint8_t esk[32];                 /* the initiator's ephemeral private key */
    uint32_t peer;                   /* row of peers; RG_PEER_NONE = empty, failed or consumed */
    uint32_t sender;                 /* our session id, msg[4..8] of the initiation */
    uint8_t pad[24];
} rg_hs_pending;

/* rg_handshake_initiate_batch_dev: encrypt_handshake_init (rustyguard-crypto/src/lib.rs:287-344) for n rows.
 * Per row, in this order:
 *   gate && gate[i] != RG_PKT_OK                       RG_PKT_REJECTED; nothing of the row is read or written
 *   peer_idx[i] >= npeers                              RG_PKT_INVALID
 *   es = X25519(esk[i], peer.public_key) all zero      RG_PKT_KEYEXCHANGE
 *   ss = X25519(own.private_key, peer.public_key)
 *   all zero                                           RG_PKT_KEYEXCHANGE
 *   otherwise                                          RG_PKT_OK: messages[i] = the 148-byte HandshakeInit
 *       le32(1) || session_ids[i] || X25519(esk[i], 9) || sealed own.public_key (48) || sealed timestamps[i]
 *       (28) || mac1 || mac2 (12 zero bytes behind it), mac1 under peers[p].mac1_key over bytes 0..116, mac2
 *       under cookies[i] over bytes 0..132 when cookies && has_cookie[i], else zero; pending[i] = the
 *       handshake state, esk[i], p and session_ids[i].
 * On a failure the message row is 160 zero bytes and the pending row is zero with peer = RG_PEER_NONE; a lane
 * stores its status after its rows.  has_cookie is required with cookies.  The per-peer ss secret is computed
 * by every row (no secret table in this interface). */
int rg_handshake_initiate_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers, uint32_t npeers,
                                    const uint32_t *peer_idx /* [n] */, const uint8_t *gate /* [n] or NULL */,
                                    const uint8_t *esk /* [n][32] */, const uint8_t *timestamps /* [n][12] TAI64N */,
                                    const uint32_t *session_ids /* [n] */,
                                    const uint8_t *cookies /* [n][16] or NULL */,
                                    const uint8_t *has_cookie /* [n], required with cookies */, size_t n,
                                    uint8_t *messages /* [n][160], 16-byte aligned, 148 bytes used */,
                                    rg_hs_pending *pending /* [n] */, uint8_t *status, void *stream);

/* rg_handshake_finish_batch_dev: decrypt_handshake_resp (lib.rs:435-465) and HandshakeState::split(true)
 * (prim.rs:299-313) for n messages against npending pending rows.  pend_table maps a receiver id (the
 * `sender` of a pending row) to its row: an rg_rx_table_build table over those words.  desc[i]: offset, len =
 * whole message.  Per message, in this order:
 *   offset % 16 != 0                                   RG_PKT_UNALIGNED
 *   frame outside [buf, buf + buf_len), or len != 92   RG_PKT_INVALID
 *   gate && gate[i] != RG_PKT_OK, or
 *   key_idx == RG_KEY_SKIP                             RG_PKT_REJECTED, message not read
 *   type word != 2                                     RG_PKT_INVALID
 *   msg[8..12] not in pend_table, or its row's
 *   peer == RG_PEER_NONE                               RG_PKT_REJECTED (handshake.rs:171-189: no session, or
 *                                                      one already past the handshake)
 *   table row >= npending, or the row's peer >= npeers RG_PKT_INVALID
 *   ee = X25519(pending.esk, msg[12..44]) all zero     RG_PKT_KEYEXCHANGE
 *   se = X25519(own.private_key, msg[12..44]) all zero RG_PKT_KEYEXCHANGE
 *   the empty field's tag fails                        RG_PKT_DECRYPT_ERR
 *   a lower-indexed message of this batch finished
 *   the same pending row                               RG_PKT_REJECTED
 *   otherwise                                          RG_PKT_OK: transport_keys[i] = send key || receive key
 *       (send = the new chain, receive = HKDF's second output: the mirror of the response call's row),
 *       pend_idx_out[i] = the pending row, remote_out[i] = msg[4..8] -- what rg_sessions_insert takes -- and
 *       the pending row is wiped (zeros, peer = RG_PEER_NONE: hs.zeroize()), so a row is consumed once.
 * On a failure the key row is zero, pend_idx_out[i] = RG_PEER_NONE and remote_out[i] = 0.  mac1 and mac2 are
 * NOT checked here: run rg_cookie_reply_batch_dev first and pass its status as gate.  buf is never written.
 *
 * "First finisher wins" is the reference's in-order loop; here it takes two launches and no ordering by
 * arrival.  The call fills claim[npending] (a workspace of the call) with 0xFFFFFFFF; the finish kernel reads
 * pending rows and never writes them, leaves every message whose tag opened at RG_PKT_PENDING and takes
 * atomicMin(&claim[row], i); a commit kernel then gives RG_PKT_OK to the lane with claim[row] == i, which
 * wipes the row, and RG_PKT_REJECTED (zero outputs) to every other pending lane.  A minimum does not depend
 * on the order the lanes arrive in, so the result is deterministic, and nothing reads RG_PKT_OK before the
 * lane that decided it wrote it.
 *
 * One deliberate difference from the reference: decrypt_handshake_resp mixes into the session's
 * HandshakeState in place before it can fail, so there a response that fails its tag leaves the pending
 * handshake corrupted.  Here a failing message leaves the pending row untouched, and a later valid response,
 * in this batch or the next, still finishes it: a forged response must not be able to kill a handshake, and
 * the corrupted state would depend on the order of arrival.
 *
 * RG_EINVAL also for pend_cap not a power of two. */
int rg_handshake_finish_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers, uint32_t npeers,
                                  const rg_rx_entry *pend_table, uint32_t pend_cap, rg_hs_pending *pending,
                                  uint32_t npending, const rg_pkt_desc *desc, const uint8_t *gate /* [n] or NULL */,
                                  size_t n, const uint8_t *buf, size_t buf_len,
                                  uint8_t *transport_keys /* [n][64]: send key || receive key */,
                                  uint32_t *pend_idx_out /* [n] */, uint32_t *remote_out /* [n] */,
                                  uint32_t *claim /* [npending] workspace */, uint8_t *status, void *stream);

/* ------------------------------ per-peer handshake state on the device (batch, async) */
/* The three fields the reference keeps per peer around a handshake (Peer, rustyguard-core/src/lib.rs:170-180) as
 * a device table, one row per row of rg_hs_peer, so that the responder chain and the initiator's cookie loop run
 * on one stream with no host step and can be captured into a graph.  A zeroed row is Peer::new.  The caller owns
 * the table; the library reads and writes only the rows a batch names.  Cookies are never expired here, as in
 * the reference (WireGuard's 120 s rule is the caller's: clear has_cookie).
 *
 * The conventions are the handshake calls': all pointers are device memory; the calls enqueue on `stream` and
 * return without waiting and keep nothing in the context; n == 0 returns RG_OK; RG_EINVAL with nothing enqueued
 * for a null required pointer (state, cookie_keys and claim are required when npeers > 0), n > 2^32 - 1, a
 * misaligned array or a short workspace.  state and struct rows must be 16-byte aligned, word arrays (peers_out,
 * peer_idx, cookies_out, claim, sess_table) 4-byte aligned.  A lane stores its status after everything else
 * it writes.
 *
 * The chains, each on one stream (the existing calls take the new arrays as they are):
 *   responder: rg_cookie_reply_batch_dev -> rg_handshake_init_batch_dev (gate = the filter's status) ->
 *     rg_peer_ts_batch_dev -> rg_peer_cookies_batch_dev (peers_out) -> rg_handshake_resp_batch_dev (gate = status)
 *     -> rg_peer_mac1_batch_dev (peers_out, responses, 96, 60)
 *   initiator: rg_peer_cookies_batch_dev (peer_idx) -> rg_handshake_initiate_batch_dev -> rg_peer_mac1_batch_dev
 *     (peer_idx, messages, 160, 116); later, on the incoming type-3 messages, rg_peer_cookie_consume_batch_dev
 *     (gate = the status of whatever admission filter the caller runs, or NULL: a CookieMessage carries no mac). */
typedef struct rg_hs_peer_state {    /* 64 bytes, 16-byte aligned rows */
    uint8_t latest_ts[12];           /* peer.latest_ts: the newest TAI64N an initiation of this peer carried */
    uint32_t has_cookie;             /* 0 or 1: peer.cookie is Some */
    uint8_t cookie[16];              /* peer.cookie */
    uint8_t last_sent_mac1[16];      /* peer.last_sent_mac1: the AAD of a cookie reply to what we sent last */
    uint8_t pad[16];
} rg_hs_peer_state;

/* rg_peer_ts_batch_dev: the timestamp-replay check of handle_handshake_init (handshake.rs:88-91) for the rows
 * rg_handshake_init_batch_dev just wrote, in place.  A row is eligible iff status[i] == RG_PKT_OK and
 * results[i].peer < npeers.  The outcome equals, bit for bit, this loop over the eligible rows in array order:
 *     if results[i].timestamp < state[p].latest_ts (as bytes, i.e. big-endian)   RG_PKT_REJECTED
 *     else state[p].latest_ts = results[i].timestamp                             stays RG_PKT_OK
 * An equal timestamp passes (the reference compares with <).  Every other row:
 *   status[i] != RG_PKT_OK                            keeps its status
 *   RG_PKT_OK with results[i].peer >= npeers          RG_PKT_INVALID
 * A row this call turns down (rejected or invalid) has its results row wiped to 128 zero bytes with peer =
 * RG_PEER_NONE, as the init call does for its own failures.  peers_out[i] is the peer of a row that is RG_PKT_OK
 * afterwards and RG_PEER_NONE otherwise: the peer_idx of rg_peer_cookies_batch_dev and rg_peer_mac1_batch_dev.
 *
 * No ordering by arrival: whether or not a row is accepted, latest after it is max(latest, its timestamp), so
 * row i is accepted iff its timestamp >= max(state[p].latest_ts, the timestamps of the eligible rows j < i of
 * peer p) -- a segmented exclusive prefix maximum over the rows grouped stably by peer (the core the device
 * anti-replay commit and the send reservation share), with the 96-bit timestamp as the value -- and the peer's
 * last row leaves max(latest_ts, the group's maximum) in the table.  A peer with no eligible row keeps its row
 * byte for byte.
 *
 * workspace: rg_peer_ts_workspace_size(n, npeers) bytes, 16-byte aligned, the call's scratch (0 when n is too
 * large for any workspace; non-decreasing in n and in npeers). */
size_t rg_peer_ts_workspace_size(size_t n, uint32_t npeers);
int rg_peer_ts_batch_dev(rg_ctx *ctx, rg_hs_peer_state *state, uint32_t npeers,
                         rg_hs_init_result *results /* [n], written */, uint8_t *status /* [n], in place */,
                         uint32_t *peers_out /* [n] */, size_t n, void *workspace, size_t workspace_len,
                         void *stream);

/* rg_peer_cookie_consume_batch_dev: Sessions::handle_cookie / decrypt_cookie (handshake.rs:233-257,
 * rustyguard-crypto/src/lib.rs) for n CookieMessages.  sess_table maps a receiver id (the session id of an
 * initiation or response we sent) to its peer row: an rg_rx_table_build table.  cookie_keys[p] is
 * cookie_key(peers[p].public_key) = BLAKE2s-256("cookie--" || public key) (lib.rs:75-77).  desc[i]: offset, len
 * = whole message.  Per message, in this order:
 *   offset % 16 != 0                                   RG_PKT_UNALIGNED
 *   frame outside [buf, buf + buf_len), or len != 64   RG_PKT_INVALID
 *   gate && gate[i] != RG_PKT_OK, or
 *   key_idx == RG_KEY_SKIP                             RG_PKT_REJECTED, message not read
 *   type word != 3                                     RG_PKT_INVALID
 *   msg[4..8] not in sess_table                        RG_PKT_REJECTED
 *   its peer >= npeers                                 RG_PKT_INVALID
 *   XChaCha20-Poly1305 open fails                      RG_PKT_DECRYPT_ERR
 *   otherwise                                          RG_PKT_OK, cookies_out[i] = the cookie
 * The open: key cookie_keys[p], nonce msg[8..32], AAD state[p].last_sent_mac1 as it stood before the call,
 * ciphertext msg[32..48], tag msg[48..64]; the tag comparison has no early exit.  On any failure cookies_out[i]
 * is zero.  buf is never written (the reference decrypts in place).
 *
 * Every message that opens is RG_PKT_OK, as in the reference, where a later valid cookie overwrites an earlier
 * one; the one that stays in state[p].cookie is that of the highest message index, whatever order the lanes
 * arrive in: the call zeroes claim[npeers] (a workspace of the call), every message that opened takes
 * atomicMax(&claim[p], i + 1), and a commit launch over the peers copies cookies_out[claim[p] - 1] into the row
 * and sets has_cookie = 1.  A peer with no valid message keeps its row byte for byte.  The call writes only
 * cookie and has_cookie and reads only last_sent_mac1.
 * RG_EINVAL also for sess_cap not a power of two; cookie_keys and desc must be 16-byte aligned. */
int rg_peer_cookie_consume_batch_dev(rg_ctx *ctx, rg_hs_peer_state *state, uint32_t npeers,
                                     const uint8_t *cookie_keys /* [npeers][32] */, const rg_rx_entry *sess_table,
                                     uint32_t sess_cap, const rg_pkt_desc *desc, const uint8_t *gate /* [n] or NULL */,
                                     size_t n, const uint8_t *buf, size_t buf_len, uint8_t *cookies_out /* [n][16] */,
                                     uint32_t *claim /* [npeers] workspace */, uint8_t *status, void *stream);

/* rg_peer_cookies_batch_dev: the cookies / has_cookie arrays rg_handshake_initiate_batch_dev and
 * rg_handshake_resp_batch_dev take, out of the table: cookies_out[i] = state[p].cookie and has_cookie_out[i] = 1
 * for p = peer_idx[i] < npeers with has_cookie set; 16 zero bytes and 0 for every other row (RG_PEER_NONE
 * included). */
int rg_peer_cookies_batch_dev(rg_ctx *ctx, const rg_hs_peer_state *state, uint32_t npeers,
                              const uint32_t *peer_idx /* [n] */, size_t n, uint8_t *cookies_out /* [n][16] */,
                              uint8_t *has_cookie_out /* [n] */, void *stream);

/* rg_peer_mac1_batch_dev: peer.last_sent_mac1 after a send (handshake.rs:108, new_handshake).  For every row with
 * status[i] == RG_PKT_OK and p = peer_idx[i] < npeers: state[p].last_sent_mac1 = the 16 bytes at messages +
 * i * stride + mac1_offset; of several rows of one peer the highest i stays (the in-order result), by atomicMax
 * into claim[npeers] (zeroed by the call) and a commit launch over the peers.  The initiator passes (160, 116),
 * the responder (96, 60).  RG_EINVAL unless mac1_offset % 4 == 0 and mac1_offset + 16 <= stride. */
int rg_peer_mac1_batch_dev(rg_ctx *ctx, rg_hs_peer_state *state, uint32_t npeers, const uint32_t *peer_idx /* [n] */,
                           const uint8_t *status /* [n] */, const uint8_t *messages, uint32_t stride,
                           uint32_t mac1_offset, size_t n, uint32_t *claim /* [npeers] workspace */, void *stream);

/* Tuning knobs.  lanes: lanes cooperating on one packet (0 = automatic, else
 * 1/2/4).  wg_per_cu: resident 256-thread workgroups per CU of the persistent
 * grid (0 = automatic, -1 = plain one-shot grid). */
int rg_set_lanes_per_packet(rg_ctx *ctx, int lanes);
int rg_get_lanes_per_packet(rg_ctx *ctx, size_t n);
int rg_set_wg_per_cu(rg_ctx *ctx, int wg_per_cu);
/* Kernel choice: -1 (default) = automatic by batch size (rg_get_kernel);
 * 0 = pipelined lane kernel (one packet -- or one of lanes_per_packet
 * contiguous segments -- per lane, 3 chunks in flight, Poly1305 folded
 * into the keystream rounds); 1/2 = LDS-staged tiles (one packet (segment) per
 * lane, coalesced LDS-DMA windows of that many 64-byte chunks); 3 = flattened
 * chunk stream (a wave takes a run of whole packets of equal total work and
 * deals their 64-byte chunks evenly over its lanes; Poly1305 partial sums are
 * combined per packet in LDS). */
int rg_set_staged(rg_ctx *ctx, int kernel);
/* The kernel family a batch of n packets runs on (0, 1 or 2; see above).  In automatic mode a
 * small batch whose sizes are mixed (the last planned batch of the same planner -- the device API's,
 * or a host pipeline slot's -- held more than one size class) runs family 3 instead, the flattened
 * chunk stream (rg_set_staged(ctx, 3) forces it); every 32nd such call re-plans on family 0. */
int rg_get_kernel(rg_ctx *ctx, size_t n);
/* The family the most recent batched launch on this context ran (-1 before any). */
int rg_last_kernel(rg_ctx *ctx);
/* A device-side planner can first sort the batch into size classes so that
 * every 64-lane tile holds packets of similar length (both kernel families;
 * the pipelined kernel then also picks segments per class by an estimated
 * makespan and deals tiles heaviest first, in snake order over the SIMDs).
 * 0 = off (tiles take packets in array order), 1 = always, 2 (default) =
 * auto: plan unless the last planned batch of this context held a single size
 * class (re-checked every 32nd call).  Results are identical in every mode.
 * Device-API calls that share a context use one set of planner buffers and one
 * tile-kernel work pool (batches of eight or more deal rounds, CUs x 4 Ki packets =
 * 1 Mi on 256 CUs, even with the planner off): two device-API launches on one
 * context on different streams are unsupported at any batch size -- issue them on
 * one stream (or order them).  The host-memory API has its own per pipeline stream. */
int rg_set_plan(rg_ctx *ctx, int on);
/* Segments per packet for the tile kernels: 0 (default) = per size class,
 * aiming at two resident waves per SIMD; 1/2/4 = split every packet into that
 * many contiguous segments on separate waves (Poly1305 partial sums combined
 * as sum_j A_j r^{N_j}). */
int rg_set_segments(rg_ctx *ctx, int segments);
/* Diagnostics.  The product library accepts only mode 0 and a NULL stamp buffer
 * (RG_EINVAL otherwise): no context of it can emit frames that are not sealed.
 * Diagnostic builds (-DRG_DIAG, tools/build_variant.sh, never shipped) add seal
 * modes whose output is NOT a valid seal -- 1 compute only (no payload
 * loads/stores), 2 memory only, 4/5/6 non-temporal loads / stores / both,
 * 7 no payload stores, 8 line stores alternating between two lines per frame
 * (pipelined kernel) -- and mode 3, per-wave stamps of the real kernels. */
int rg_set_debug_mode(rg_ctx *ctx, int mode);
/* Diagnostic builds only: per-wave s_memtime stamps are written to this device
 * buffer, 8 x u64 per wave: mode 3 on the tile kernels (setup, store,
 * dma-issue, dma-wait, chunk, tail, valid, real-time ticks at 100 MHz); any
 * non-zero mode on the pipelined kernel (cycles, two unit marks, XCC_ID << 32 |
 * HW_ID, start tick, prologue cycles, valid, real-time ticks); mode 3 on the
 * flattened kernel (s_memtime at the end of each phase) plus a second block of
 * rows after the first CUs x 4 (wall-clock start and end, the unit search's
 * steps) and a third (the first sub-unit's packets / chunks / steps, XCC_ID << 32
 * | HW_ID), so size the buffer for 3 x CUs x 4 x 8 u64 there. */
int rg_set_debug_buffer(rg_ctx *ctx, void *dev_ptr);

/* ----------------------------------------- host-memory batch (blocking) */
/* Same contract with host pointers: frames are staged H2D, sealed/opened on
 * the GPU and copied back D2H, pipelined over three streams.  Pinned memory
 * (rg_host_alloc) gives the full PCIe rate.  rg_set_host_slice sets the byte
 * span of one pipeline slice (default 8 MiB; 64 KiB .. 1 GiB).
 *
 * Every host wait of the library is bounded: a completion the device does not
 * report within rg_set_wait_timeout's limit (default 10 000 ms per wait; 1 ..
 * 3 600 000) ends the call with RG_EDEVICE ("... timed out") and every status
 * RG_PKT_PENDING, instead of blocking forever.  Waits poll (hipEventQuery),
 * yielding the CPU between polls and sleeping once a wait has run 2 ms.  The
 * transfers of a timed-out call may still complete later: until the next host
 * call on that context returns (it waits for them, bounded, and discards them),
 * the frames of the failed call's buffer can still be written back. */
int rg_set_host_slice(rg_ctx *ctx, size_t bytes);
int rg_set_wait_timeout(rg_ctx *ctx, uint32_t ms);
int rg_seal_batch_host(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                       const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *buf, size_t buf_len,
                       uint8_t *status);
int rg_open_batch_host(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys, const rg_pkt_desc *desc, size_t n,
                       uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out);
void *rg_host_alloc(size_t bytes);
void rg_host_free(void *p);

/* NUMA placement (a two-socket host: half the GPUs hang off each socket).  rg_numa_node: the host NUMA
 * node closest to the context's GPU (-1 unknown).  A group's worker thread for a context runs on the CPUs
 * of that node this process may use and prefers its memory for the slice buffers it allocates.  Frames
 * are the caller's: for the full link rate a caller that owns a batch's buffer (a UDP ring, say) places
 * each context's part -- rg_split_batch's bounds -- on that context's node, by first touch from a thread
 * there or with rg_numa_bind (mbind MPOL_BIND + MPOL_MF_MOVE over the pages covering [p, p + bytes)), then
 * pins it with rg_host_register (hipHostRegister; rg_host_unregister before freeing).  Pinned pages do not
 * move: bind first. */
int rg_numa_node(rg_ctx *ctx);
int rg_numa_bind(void *p, size_t bytes, int node);
int rg_host_register(void *p, size_t bytes);
int rg_host_unregister(void *p);

/* ------------------------- per-message drop-in for CryptoPrimatives */
/* Exactly Core::chacha20poly1305_enc / _dec (prim.rs:179-201): any nonce,
 * any AAD, any length up to RFC 8439's 64 * (2^32 - 1) bytes (a longer
 * one is RG_EINVAL), host pointers, blocking.  dec returns RG_OK, or
 * RG_PKT_DECRYPT_ERR (positive 1) on a tag mismatch with payload untouched. */
int rg_chacha20poly1305_enc(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[12], const uint8_t *aad,
                            size_t aad_len, uint8_t *payload, size_t len, uint8_t tag[16]);
int rg_chacha20poly1305_dec(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[12], const uint8_t *aad,
                            size_t aad_len, uint8_t *payload, size_t len, const uint8_t tag[16]);

/* Core::xchacha20poly1305_enc / _dec (prim.rs:202-224; decl :97-110), the
 * cookie-reply AEAD (encrypt_cookie / decrypt_cookie, rustyguard-crypto/src/
 * lib.rs:50-70): HChaCha20(key, nonce[0..16]) subkey, then ChaCha20-Poly1305
 * with nonce 0^4 || nonce[16..24].  Same contract as the pair above. */
int rg_xchacha20poly1305_enc(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[24], const uint8_t *aad,
                             size_t aad_len, uint8_t *payload, size_t len, uint8_t tag[16]);
int rg_xchacha20poly1305_dec(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[24], const uint8_t *aad,
                             size_t aad_len, uint8_t *payload, size_t len, const uint8_t tag[16]);

/* ---------------------------------------------- host-side session layer */
/* AntiReplay: RFC 6479 window, 2048-bit bitmap, WINDOW_SIZE = 1984
 * (rustyguard-utils/src/anti_replay.rs:1-64), identical semantics. */
typedef struct rg_antireplay {
    uint64_t bitmap[32];
    uint64_t last;
} rg_antireplay;
#define RG_REPLAY_WINDOW 1984u

void rg_antireplay_init(rg_antireplay *r);
int rg_antireplay_would_accept(const rg_antireplay *r, uint64_t n);
void rg_antireplay_mark_seen(rg_antireplay *r, uint64_t n);

/* Session table: the transport half of rustyguard_core::Sessions.  Each
 * session owns an EncryptionKey {key, counter} and a DecryptionKey {key,
 * AntiReplay} (prim.rs:376-437), the peer's receiver id for outgoing
 * headers, and our local id that incoming headers name
 * (rustyguard-core/src/lib.rs:230-235, :646-650). */
typedef struct rg_sessions rg_sessions;

/* REKEY_AFTER_MESSAGES / REJECT_AFTER_MESSAGES, rustyguard-core/src/lib.rs:63-65 */
#define RG_REKEY_AFTER_MESSAGES (1ull << 60)
#define RG_REJECT_AFTER_MESSAGES (0xFFFFFFFFFFFFFFFFull - (1ull << 13))
/* KEEPALIVE_TIMEOUT / REKEY_AFTER_TIME / REJECT_AFTER_TIME, rustyguard-core/src/lib.rs:66-70, in nanoseconds */
#define RG_KEEPALIVE_TIMEOUT_NS 10000000000ull
#define RG_REKEY_AFTER_TIME_NS 120000000000ull
#define RG_REJECT_AFTER_TIME_NS 180000000000ull

int rg_sessions_create(rg_ctx *ctx, uint32_t capacity, rg_sessions **out);
void rg_sessions_destroy(rg_sessions *s);
/* Install a transport session (HandshakeState::split output, prim.rs:299-313);
 * returns the slot index (>= 0) or a negative rg_status.  The session is its own peer
 * (its endpoint is its own); rg_sessions_insert_peer names the peer. */
int rg_sessions_insert(rg_sessions *s, uint32_t local_id, uint32_t remote_id, const uint8_t send_key[32],
                       const uint8_t recv_key[32]);
/* rg_sessions_insert for a session of peer `peer` (any caller-chosen id but RG_PEER_NONE): the
 * peer's sessions -- its current transport and the ones a rekey leaves behind -- share one endpoint
 * record, as the reference keeps peer.endpoint per peer (PeerState, rustyguard-core/src/lib.rs:
 * 160-181, set by decrypt_packet at :670-671, read by the Keepalive timer, time.rs:135).  The
 * peer's record outlives its sessions (a new session of a known peer starts with its endpoint). */
#define RG_PEER_NONE 0xFFFFFFFFu
int rg_sessions_insert_peer(rg_sessions *s, uint32_t local_id, uint32_t remote_id, const uint8_t send_key[32],
                            const uint8_t recv_key[32], uint32_t peer);
int rg_sessions_remove(rg_sessions *s, uint32_t slot);
int rg_sessions_lookup(const rg_sessions *s, uint32_t local_id); /* slot or RG_ENOTFOUND */
/* EncryptionKey::counter() (prim.rs:396-398) / overwrite, e.g. for REKEY tests */
uint64_t rg_sessions_send_counter(const rg_sessions *s, uint32_t slot);
int rg_sessions_set_send_counter(rg_sessions *s, uint32_t slot, uint64_t counter);
rg_antireplay *rg_sessions_replay(rg_sessions *s, uint32_t slot);

/* Batched PeerState::encrypt_message + frame_in_place over host frames.
 * Packets are processed in array order: each takes the next counter of its
 * session (EncryptionKey::encrypt, prim.rs:386-394) and sets its sent time.  status[i]:
 * OK, INVALID (P % 16 != 0 / bad desc), REJECTED (counter >= REJECT_AFTER_MESSAGES or
 * the session older than REJECT_AFTER_TIME, lib.rs:204-209, 260-262).  rekey_out[i]
 * (nullable) = 1 when the session counter reached REKEY_AFTER_MESSAGES (lib.rs:564-570). */
int rg_send_batch(rg_sessions *s, const uint32_t *slots, const rg_pkt_desc *desc, size_t n, uint8_t *buf,
                  size_t buf_len, uint8_t *status, uint8_t *rekey_out);
/* Batched Sessions::recv_message for data frames: alignment/type/length
 * checks, receiver-id -> session, replay pre-filter, GPU open, then the
 * in-order anti-replay post-pass (A6 in SURVEY.md §8): packet j is accepted
 * iff its tag verifies and would_accept(n_j) holds after packets 0..j-1.
 * slots_out[i] = session slot (or 0xFFFFFFFF). */
int rg_recv_batch(rg_sessions *s, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                  uint8_t *status, uint32_t *slots_out);

/* rg_recv_batch with decrypt_packet's side effects (rustyguard-core/src/lib.rs:664-679):
 * src[i] (nullable) is an opaque tag of packet i's source address; for every packet that is
 * authenticated and accepted, in array order, the session's endpoint becomes src[i] (only
 * authenticated packets move it: whitepaper §6.5, the reference's recv_message fuzz
 * invariant) and flags_out[i] (nullable) gets RG_RECV_AUTHENTICATED, plus RG_RECV_KEEPALIVE
 * when sent + KEEPALIVE_TIMEOUT < now and no keepalive is pending yet (the caller schedules
 * the Keepalive timer; rg_sessions_keepalive_due runs it).  Other packets get flags 0. */
#define RG_RECV_AUTHENTICATED 1u
#define RG_RECV_KEEPALIVE 2u
int rg_recv_batch_ex(rg_sessions *s, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                     const uint64_t *src, uint8_t *status, uint32_t *slots_out, uint8_t *flags_out);
/* The table's clock: Sessions::turn's state.now (lib.rs:396-413) as monotonic nanoseconds.
 * Sessions take it as started / sent when inserted; rg_send_batch sets sent and rejects
 * once started + REJECT_AFTER_TIME (180 s) < now (should_expire, lib.rs:207-209). */
void rg_sessions_set_time(rg_sessions *s, uint64_t now_ns);
/* the endpoint tag of the last authenticated packet of the session's peer (any of the peer's
 * sessions, rg_sessions_insert_peer; the session itself when inserted without a peer);
 * RG_ENOTFOUND before any.  rg_peer_endpoint reads a peer's record directly. */
int rg_sessions_endpoint(const rg_sessions *s, uint32_t slot, uint64_t *src_out);
int rg_peer_endpoint(const rg_sessions *s, uint32_t peer, uint64_t *src_out);
/* the Keepalive timer entry (rustyguard-core/src/time.rs:114-141): clears keepalive_pending
 * and returns 1 when sent + KEEPALIVE_TIMEOUT < now (should_keepalive, lib.rs:201-203): the
 * caller then seals an empty payload (P = 0) for the session with rg_send_batch. */
int rg_sessions_keepalive_due(rg_sessions *s, uint32_t slot);
/* rg_sessions_keepalive_due with the address the keepalive goes to: the session's peer endpoint
 * (peer.endpoint, time.rs:135) in *dst_out when due.  Returns 1 (due, *dst_out set), 0 (not
 * due), RG_ENOTFOUND (due but the peer never authenticated a packet: the reference's
 * "should not be scheduled" expect) or another negative rg_status. */
int rg_sessions_keepalive(rg_sessions *s, uint32_t slot, uint64_t *dst_out);

/* Device-resident variants of rg_send_batch / rg_recv_batch_ex: frames, descriptors and
 * statuses in device memory, the session state on the host.  Work is enqueued on `stream`
 * (hipStream_t) and the calls return without waiting for the GPU; the table keeps device
 * mirrors of its keys, receivers and a receiver-id -> session table, refreshed (after the
 * device work that reads them has drained) on the first device call after a session change.
 *
 * rg_send_batch_dev: slots[] and rekey_out[] are host arrays; desc[i].key_idx is ignored
 * (the packet's session decides it).  Counters are reserved on the host in array order as
 * rg_send_batch does; since the lengths are on the device, a frame with P % 16 != 0 still takes
 * a counter and the kernel reports it RG_PKT_INVALID (nonces stay unique).  status (device,
 * required as for rg_seal_batch_dev) gets the per-packet statuses.  Two sends may be in flight; a
 * third waits for the first one's seal. */
int rg_send_batch_dev(rg_sessions *s, const uint32_t *slots, const rg_pkt_desc *desc, size_t n, uint8_t *buf,
                      size_t buf_len, uint8_t *status, uint8_t *rekey_out, void *stream);
/* rg_recv_batch_dev enqueues receiver resolution (rg_open_batch_dev_rx), the GPU open and
 * the copy of (status, counter, session) per packet to pinned host memory; status (device)
 * gets the GPU verdicts.  rg_recv_batch_dev_finish waits for that copy, runs the in-order
 * anti-replay pass and decrypt_packet's side effects exactly as rg_recv_batch_ex (src, flags),
 * writes the final statuses back to the device status array, and re-seals frames it rejected
 * (they go back to ciphertext), all on the batch's stream; status_out / slots_out / flags_out
 * are optional host arrays.  One device receive may be pending per table: finish it before
 * the next rg_recv_batch_dev, rg_sessions_insert or rg_sessions_remove (RG_EINVAL otherwise).
 * Replayed frames are decrypted and re-sealed (the device cannot consult the window first). */
int rg_recv_batch_dev(rg_sessions *s, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                      uint8_t *status, void *stream);
int rg_recv_batch_dev_finish(rg_sessions *s, const uint64_t *src, uint8_t *status_out, uint32_t *slots_out,
                             uint8_t *flags_out);

/* ------------------------------ device-resident anti-replay (async) */
/* The RFC 6479 windows in device memory beside the key table, and a receive that never leaves the stream.
 * Window state is rg_antireplay as defined above, one row per key-table row, 8-byte aligned, owned by the
 * caller (hipMemset 0 = rg_antireplay_init).  All pointers are device memory; the calls enqueue on `stream`
 * and return without waiting, allocate nothing and keep nothing in the context (so they can be captured
 * into a graph): every scratch array lives in `workspace`, 16-byte aligned, of at least
 * rg_replay_workspace_size(n, nwin) bytes (0 when n is too large for any workspace; non-decreasing in both
 * arguments).  A workspace belongs to one call at a time: the next call on the same stream may reuse it.
 *
 * rg_replay_batch_dev is the in-order tail of DecryptionKey::decrypt (prim.rs:414-437) for a batch.  Its
 * result equals, bit for bit (status, undo and every byte of every window), this loop over the host
 * functions above:
 *   for i in 0..n, in array order:
 *     w = win_idx[i]
 *     if w == RG_KEY_SKIP or w >= nwin or status[i] is neither RG_PKT_OK nor RG_PKT_DECRYPT_ERR:
 *         status[i] stays; undo[i] = 0                       (RG_PKT_PENDING is never turned into a verdict)
 *     elif !rg_antireplay_would_accept(&windows[w], counters[i]):
 *         undo[i] = (status[i] == RG_PKT_OK); status[i] = RG_PKT_REJECTED     (also when the tag was bad)
 *     elif status[i] == RG_PKT_OK:
 *         rg_antireplay_mark_seen(&windows[w], counters[i]); undo[i] = 0
 *     else: undo[i] = 0                                      (stays RG_PKT_DECRYPT_ERR, window untouched)
 * computed in parallel, also within one window (a segmented prefix maximum over each window's packets, a
 * (window, counter) table for duplicates inside the batch).  undo may be NULL.
 *
 * rg_recv_batch_dev_resident is Sessions::decrypt_packet's transport half with no host step: receiver
 * resolution (as rg_open_batch_dev_rx), the would_accept pre-check of prim.rs:414-420 against the windows as
 * they stand before the batch (a frame that fails it reaches the open kernels as RG_KEY_SKIP: RG_PKT_REJECTED,
 * no AEAD work, frame untouched -- exact, since a counter a window rejects is rejected by every later state
 * of it), the open, the in-order commit above, and the re-seal of frames the open decrypted and the commit
 * then rejected (byte for byte back to ciphertext, as rg_recv_batch_dev_finish does) -- all enqueued on
 * `stream`, nothing waited for.  windows[nkeys] runs parallel to the key table.  status gets the FINAL
 * verdicts (those rg_recv_batch_ex gives for the same frames and windows); counters_out / key_idx_out (may
 * be NULL) as rg_open_batch_dev_rx, except that a gated packet still reports its header counter and its
 * resolved key row.  The workspace begins with the call's n working descriptors (rg_pkt_desc rows: the
 * caller's descriptors with the key row the open ran under, RG_KEY_SKIP for a frame without a session or one
 * the gate turned away), which a caller may read behind the call.  The call runs the context's open and seal kernels and so shares its planner buffers
 * with the other device calls: the one-stream rule above applies (a call on another stream while the
 * context's last batch is in flight fails with RG_EINVAL, nothing enqueued), and a buffer of the context
 * that has to grow does so outside a stream capture (run the shape once before capturing it).  The endpoint
 * side effect of decrypt_packet (lib.rs:670-679) is rg_endpoint_note_recv_batch_dev behind this call, on its
 * status and key_idx_out; the keepalive side effect (:664-669) is rg_timer_note_recv_batch_dev, likewise.
 *
 * n == 0 returns RG_OK.  RG_EINVAL, nothing enqueued: a null required pointer (undo, counters_out and
 * key_idx_out are optional), n > 2^32 - 1, windows not 8-byte or workspace not 16-byte aligned,
 * workspace_len smaller than rg_replay_workspace_size reports; for the receive also nkeys == 0 or rx_cap
 * not a power of two. */
size_t rg_replay_workspace_size(size_t n, uint32_t nwin);
int rg_replay_batch_dev(rg_ctx *ctx, rg_antireplay *windows, uint32_t nwin, const uint32_t *win_idx,
                        const uint64_t *counters, size_t n, uint8_t *status, uint8_t *undo, void *workspace,
                        size_t workspace_len, void *stream);
int rg_recv_batch_dev_resident(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys, const rg_rx_entry *rx_table,
                               uint32_t rx_cap, rg_antireplay *windows, const rg_pkt_desc *desc, size_t n,
                               uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out,
                               uint32_t *key_idx_out, void *workspace, size_t workspace_len, void *stream);

/* ------------------------------------ device-resident send (async) */
/* The send counters in device memory beside the key table, and a send that never leaves the stream: the
 * transmit half of the section above, with the same conventions.  One rg_send_state row per key-table row,
 * 8-byte aligned, owned by the caller (a new session: counter = 0, started_ns = sent_ns = its start time).
 * All pointers are device memory; the calls enqueue on `stream` and return without waiting, allocate nothing
 * and keep nothing in the context (so they can be captured into a graph): every scratch array lives in
 * `workspace`, 16-byte aligned, of at least rg_send_workspace_size(n, nkeys) bytes (0 when n is too large for
 * any workspace; non-decreasing in both arguments).  A workspace belongs to one call at a time: the next
 * call on the same stream may reuse it.  slots[i] is packet i's key-table row; desc[i].key_idx is ignored.
 * now_ns points to one u64 in device memory, read when the kernels run (a captured graph sees each replay's
 * clock); NULL: no time rule, and sent_ns is left untouched.
 *
 * rg_send_reserve_batch_dev is the counter pass alone: the sequential part of EncryptionKey::encrypt
 * (prim.rs:386-394) and PeerState::force_encrypt (lib.rs:260-297) for a batch.  Its result equals, bit for
 * bit (status, counters_out, rekey_out and every byte of every state row), rg_send_batch's loop over the
 * device state:
 *   for i in 0..n, in array order:
 *     w = slots[i]; rekey_out[i] = 0; counters_out[i] = 0
 *     if w == RG_KEY_SKIP or w >= nkeys:                         status[i] = RG_PKT_REJECTED
 *     elif desc[i].len % 16 != 0:                                status[i] = RG_PKT_INVALID   (takes no counter)
 *     elif state[w].counter >= RG_REJECT_AFTER_MESSAGES
 *       or (now_ns and state[w].started_ns + 180e9 < *now_ns):   status[i] = RG_PKT_REJECTED  (u64 wrapping add)
 *     else: counters_out[i] = state[w].counter++; if now_ns: state[w].sent_ns = *now_ns
 *           rekey_out[i] = state[w].counter >= RG_REKEY_AFTER_MESSAGES
 *           status[i] = RG_PKT_PENDING       (a counter is reserved; only a seal lane may write RG_PKT_OK)
 * computed in parallel, also within one row, and never by atomics in arrival order: a stable grouping of the
 * packets by row and a segmented count of the eligible ones give each packet its rank.  rekey_out
 * may be NULL.  The workspace begins with the call's n working descriptors (rg_pkt_desc rows: the caller's
 * descriptors with key_idx = w, RG_KEY_SKIP for every packet that took no counter), which a caller may read
 * behind the call or hand to rg_seal_batch_dev with counters_out.
 *
 * rg_send_batch_dev_resident is that pass followed by rg_seal_batch_dev over the working descriptors and the
 * reserved counters (header from receivers[w], encrypted in place, tag written), all enqueued on `stream`,
 * nothing waited for.  state[nkeys] runs parallel to the key table.  status gets the FINAL verdicts: the
 * pass's RG_PKT_REJECTED / RG_PKT_INVALID (frame untouched), otherwise what the seal kernel wrote -- also
 * RG_PKT_UNALIGNED / RG_PKT_INVALID for a misaligned or out-of-bounds frame, which has consumed its counter
 * exactly as in rg_send_batch (nonces stay unique).  counters_out and rekey_out may be NULL.  The call runs
 * the context's seal kernels and so shares its planner buffers with the other device calls: the one-stream
 * rule above applies (a call on another stream while the context's last batch is in flight fails with
 * RG_EINVAL, nothing enqueued), and a buffer of the context that has to grow does so outside a stream
 * capture (run the shape once before capturing it).  The keepalive and rekey timers are the session-timer
 * section's: rg_timer_note_send_batch_dev behind this call, rg_timer_turn_dev when the caller turns.
 *
 * n == 0 returns RG_OK.  RG_EINVAL, nothing enqueued: a null required pointer (now_ns and rekey_out are
 * optional, for the resident call also counters_out), n > 2^32 - 1, state not 8-byte or workspace not 16-byte
 * aligned, workspace_len smaller than rg_send_workspace_size reports; for the resident call also nkeys == 0. */
typedef struct rg_send_state {
    uint64_t counter;    /* EncryptionKey.counter: the next counter to hand out */
    uint64_t started_ns; /* Session.started (REJECT_AFTER_TIME, lib.rs:204-209) */
    uint64_t sent_ns;    /* Session.sent (force_encrypt, lib.rs:285; read by the keepalive rule) */
} rg_send_state;         /* 24 bytes */

size_t rg_send_workspace_size(size_t n, uint32_t nkeys);
int rg_send_reserve_batch_dev(rg_ctx *ctx, rg_send_state *state, uint32_t nkeys, const uint32_t *slots,
                              const rg_pkt_desc *desc, size_t n, const uint64_t *now_ns, uint8_t *status,
                              uint64_t *counters_out, uint8_t *rekey_out, void *workspace, size_t workspace_len,
                              void *stream);
int rg_send_batch_dev_resident(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                               rg_send_state *state, const uint32_t *slots, const rg_pkt_desc *desc, size_t n,
                               const uint64_t *now_ns, uint8_t *buf, size_t buf_len, uint8_t *status,
                               uint64_t *counters_out, uint8_t *rekey_out, void *workspace, size_t workspace_len,
                               void *stream);

/* ------------------------------- device-resident cryptokey routing (async) */
/* The AllowedIPs table in device memory, so that neither direction of the resident transport path reads a
 * packet header back to the host: handle_intern's peer_net.lookup(&dest) and zero padding
 * (rustyguard-tun/src/lib.rs:214-243) ahead of the send, handle_extern's source check (:174-202) behind the
 * receive.  IPv4 only, as the reference (Ipv4LCTrieMap<PeerId>).
 *
 * The table is a fixed-stride 16-8-8 multibit trie in uint32_t words (csrc/rg_route.h and DESIGN.md have the
 * encoding): a root of 65536 entries, child blocks of 256, a lookup of at most three dependent loads.
 * rg_route_table_words gives the exact size for a prefix array (0 if a row is invalid); rg_route_table_build
 * writes it into host memory, which the caller uploads.  Lookup is longest-prefix match; no match is
 * RG_PEER_NONE (the reference's sentinel root); a /0 prefix sets the default; bits of addr below prefix_len are
 * ignored; the same (network, length) given twice takes the last row's peer; np == 0 gives the all-NONE root.
 * The build is deterministic: the table is a function of the prefix array.  There is no in-place update:
 * replacing a table is building another and passing the other pointer from the next batch on.
 * rg_route_table_build: RG_EINVAL for a null pointer (p may be NULL when np == 0), prefix_len > 32 or
 * peer > 0x7FFFFFFF; RG_EFULL when cap_words < rg_route_table_words(p, np), nothing written.
 * rg_route_lookup is the host's lookup (RG_PEER_NONE also for a null pointer or table_words < 65536); the
 * kernels compile the same text.  Every child index is checked against table_words before it is used, so a
 * corrupt table can misroute but never makes a lookup read outside the table.
 *
 * An inner packet of L bytes is acceptable IPv4 iff L >= 20, the version nibble is 4 and
 * 20 <= 4 IHL <= total_length <= L (IHL the low nibble of byte 0, total_length bytes 2-3, big endian).
 *
 * The device calls follow the two sections above: every pointer is device memory (buf 16-byte aligned), the
 * calls enqueue on `stream` and return without waiting, allocate nothing and keep nothing in the context (so
 * they can be captured into a graph).  table_words is the table's size; no lane reads past it.
 *
 * rg_route_batch_dev is handle_intern up to send_message.  peer_slot[p] is peer p's current key-table row,
 * RG_KEY_SKIP = no session.  desc[i].offset is the frame's offset (the inner packet starts at offset + 16),
 * desc[i].len the UNPADDED inner length L; desc[i].key_idx is ignored.  For every i, independently, the first
 * rule that applies:
 *   1. offset % 16 != 0                                          status[i] = RG_PKT_UNALIGNED
 *   2. offset + 16 + roundup16(L) + 16 > buf_len (64 bits, no wrap)          RG_PKT_INVALID
 *   3. the packet is not acceptable IPv4                                     RG_PKT_INVALID
 *   4. peer = lookup(destination, bytes 16-19) is RG_PEER_NONE or >= npeers  RG_PKT_UNROUTABLE
 *   5. peer_slot[peer] == RG_KEY_SKIP                                        RG_PKT_REJECTED  (no session;
 *                                   peers_out[i] = peer: whom to start a handshake with)
 *   6. otherwise RG_PKT_OK: bytes [L, roundup16(L)) of the inner packet are set to zero,
 *      slots_out[i] = peer_slot[peer], desc_out[i] = {offset, roundup16(L), slots_out[i]}, peers_out[i] = peer
 * In every other case slots_out[i] = RG_KEY_SKIP, desc_out[i] = {offset, L, RG_KEY_SKIP} and no byte of buf is
 * written; peers_out[i] = RG_PEER_NONE in cases 1-4.  peers_out may be NULL; desc_out may be desc itself.
 * slots_out and desc_out are what rg_send_batch_dev_resident takes.
 *
 * rg_route_check_batch_dev is the source check of handle_extern, behind rg_recv_batch_dev_resident on the
 * same stream: desc[n] are the frames' descriptors (offset, frame length W), key_idx[n] what the receive
 * reported in key_idx_out, slot_peer[k] the peer of key-table row k, buf is only read.  status[n] is updated
 * in place:
 *   status[i] != RG_PKT_OK                                   stays; inner_len_out[i] = 0
 *   W == 32 (a keepalive)                                    stays RG_PKT_OK; inner_len_out[i] = 0
 *   the W - 32 bytes at offset + 16 are not acceptable IPv4  RG_PKT_INVALID (also a descriptor that is
 *                                   misaligned, outside buf or has W < 32, which no receive reports as OK)
 *   lookup(source, bytes 12-15) is RG_PEER_NONE, key_idx[i] >= nkeys,
 *   or the lookup's peer != slot_peer[key_idx[i]]            RG_PKT_UNROUTABLE
 *   otherwise                                                stays RG_PKT_OK; inner_len_out[i] = total_length
 * (inner_len_out[i] = 0 for every packet that does not end RG_PKT_OK).  total_length trims the sender's zero
 * padding.  inner_len_out may be NULL.  The anti-replay windows are not touched: the reference, too, commits
 * the counter before this check.
 *
 * rg_send_batch_dev_routed is rg_route_batch_dev, writing slots_out and desc_out into the workspace, then
 * rg_send_batch_dev_resident over them with the same state, now_ns, counters_out and rekey_out, then an overlay:
 * a packet the route did not route (status != RG_PKT_OK there) keeps the route's status, has taken no counter
 * and its frame is untouched; every other packet gets the resident send's final verdict.  Frames, statuses,
 * counters and state rows equal those of the three steps called separately.  The workspace, 16-byte aligned,
 * of at least rg_route_workspace_size(n, nkeys) bytes (0 when n is too large; non-decreasing in both
 * arguments), holds the route's arrays -- it begins with the route's n working descriptors -- and the resident
 * send's workspace.  The one-stream rule of the resident send applies unchanged, as does what it says about
 * buffers of the context that have to grow.  peers_out, counters_out, rekey_out and now_ns may be NULL.
 *
 * n == 0 returns RG_OK.  RG_EINVAL, nothing enqueued: a null required pointer, n > 2^32 - 1,
 * table_words < 65536, buf not 16-byte aligned; for the routed send also nkeys == 0, state not 8-byte or
 * workspace not 16-byte aligned, workspace_len smaller than rg_route_workspace_size reports. */
typedef struct rg_route_prefix {   /* 12 bytes */
    uint8_t  addr[4];              /* network order; bits below prefix_len are ignored (masked) */
    uint32_t prefix_len;           /* 0..32 */
    uint32_t peer;                 /* <= 0x7FFFFFFF */
} rg_route_prefix;

size_t rg_route_table_words(const rg_route_prefix *p, uint32_t np);
int rg_route_table_build(const rg_route_prefix *p, uint32_t np, uint32_t *table, size_t cap_words);
uint32_t rg_route_lookup(const uint32_t *table, size_t table_words, const uint8_t addr[4]);

size_t rg_route_workspace_size(size_t n, uint32_t nkeys);
int rg_route_batch_dev(rg_ctx *ctx, const uint32_t *table, size_t table_words, const uint32_t *peer_slot,
                       uint32_t npeers, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                       uint32_t *peers_out, uint32_t *slots_out, rg_pkt_desc *desc_out, uint8_t *status,
                       void *stream);
int rg_route_check_batch_dev(rg_ctx *ctx, const uint32_t *table, size_t table_words, const uint32_t *slot_peer,
                             uint32_t nkeys, const rg_pkt_desc *desc, const uint32_t *key_idx, size_t n,
                             const uint8_t *buf, size_t buf_len, uint8_t *status, uint32_t *inner_len_out,
                             void *stream);
int rg_send_batch_dev_routed(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                             rg_send_state *state, const uint32_t *table, size_t table_words,
                             const uint32_t *peer_slot, uint32_t npeers, const rg_pkt_desc *desc, size_t n,
                             const uint64_t *now_ns, uint8_t *buf, size_t buf_len, uint32_t *peers_out,
                             uint8_t *status, uint64_t *counters_out, uint8_t *rekey_out, void *workspace,
                             size_t workspace_len, void *stream);

/* ------------------------------ device-resident session table (batch, async) */
/* The step between the handshake calls and the resident transport calls: a batch of finished handshakes becomes
 * live rows of the tables rg_send_batch_dev_resident, rg_recv_batch_dev_resident, rg_route_batch_dev and
 * rg_route_check_batch_dev take, on the stream that produced them, and sessions past their lifetime leave the
 * tables the same way -- the tails of handle_handshake_init (rustyguard-core/src/handshake.rs:110-133) and
 * handle_handshake_resp (:201-227) and the ExpireTransport timer (rustyguard-core/src/time.rs:84-98).  No key
 * leaves the device.
 *
 * The conventions are the handshake and peer-state calls': every array is device memory; the calls enqueue on
 * `stream` and return without waiting, allocate nothing and keep nothing in the context (so they can be
 * captured into a graph); n == 0 returns RG_OK; RG_EINVAL with nothing enqueued for a null required pointer
 * (gate, now_ns, rows and expired_out are optional), n > 2^32 - 1, a misaligned array, rx_cap not a power of
 * two or < 2 nkeys, or a workspace smaller than rg_session_workspace_size(n, nkeys, npeers) reports (0 when the
 * sizes are too large for any workspace; non-decreasing in each argument; n = 0 for the expire call).  The
 * workspace is 16-byte aligned and belongs to one call at a time.  A lane stores its status after everything
 * else it writes.
 *
 * rg_session_tables is a host struct of device pointers, read at call time.  The arrays are the caller's, the
 * ones the resident calls take plus local_ids.  An empty table: slot_peer, peer_slot and rx_table filled with
 * 0xFF, everything else zero.  rx_table must be current when a call starts: every call below leaves it so, and
 * a caller that seeded rows itself runs rg_session_index_dev first. */
typedef struct rg_session_tables {
    uint8_t       *send_keys;   /* [nkeys][32]  keys of rg_send_batch_dev_resident            16-B aligned */
    uint8_t       *recv_keys;   /* [nkeys][32]  keys of rg_recv_batch_dev_resident            16-B aligned */
    uint32_t      *receivers;   /* [nkeys]      the peer's id for outgoing headers                          */
    uint32_t      *local_ids;   /* [nkeys]      our id, what incoming headers name                          */
    uint32_t      *slot_peer;   /* [nkeys]      peer of the row; RG_PEER_NONE = the row is free             */
    rg_antireplay *windows;     /* [nkeys] */
    rg_send_state *send_state;  /* [nkeys] */
    rg_rx_entry   *rx_table;    /* [rx_cap]     8-byte aligned; rx_cap a power of two >= 2 nkeys           */
    uint32_t      *peer_slot;   /* [npeers]     the peer's current row; RG_KEY_SKIP = none                  */
    uint32_t nkeys, rx_cap, npeers;
} rg_session_tables;

/* rg_session_install_batch_dev.  Its result equals this loop, bit for bit on status, rows_out, transport_keys and
 * every array of the tables except the byte layout of rx_table:
 *   free = the rows r with slot_peer[r] == RG_PEER_NONE before the call, ascending
 *   seen = the local_ids of the rows that are live before the call
 *   for i in 0..n, in array order:
 *     rows_out[i] = RG_KEY_SKIP
 *     if gate && gate[i] != RG_PKT_OK: status[i] = RG_PKT_REJECTED; nothing else of row i is read or written
 *     zero transport_keys[i] once its 64 bytes are read     (a key row is consumed once, whatever follows)
 *     if peers[i] >= npeers:           status[i] = RG_PKT_INVALID
 *     elif local_ids[i] in seen:       status[i] = RG_PKT_REJECTED
 *     else: seen += local_ids[i]                            (before the capacity check)
 *       if free is exhausted:          status[i] = RG_PKT_FULL
 *       else: r = next of free
 *         send_keys[r], recv_keys[r] = transport_keys[i][0:32], [32:64]
 *         receivers[r] = remote_ids[i]; local_ids[r] = local_ids[i]; slot_peer[r] = peers[i]
 *         windows[r] = zero; send_state[r] = {0, now, now}  (now = *now_ns, 0 when now_ns is NULL)
 *         peer_slot[peers[i]] = r                           (peer.current_transport: the last in array order)
 *         rows_out[i] = r; status[i] = RG_PKT_OK
 *   rx_table = the receiver table over { (local_ids[r], r) : slot_peer[r] != RG_PEER_NONE }
 * The peer's previous row is left alone: the reference, too, keeps an old session receiving until it expires.
 * Once free runs out every later eligible row is RG_PKT_FULL, so whether a row repeats an earlier eligible row
 * does not depend on who got a row.  Computed in parallel, nothing decided by arrival order: the live ids by a
 * read of rx_table as it stands, ids inside the batch by an atomicMin of the index in a table in the workspace,
 * rows by an exclusive count of the eligible handshakes and a compaction of the free rows, peer_slot by
 * atomicMax(claim[p], i + 1) and a commit over the peers.  All n statuses are RG_PKT_PENDING first.
 *
 * rx_table is rebuilt at the end of every call that changes rows: a memset to 0xFF, then one lane per live row
 * claims the first empty entry from its home slot.  Which of two colliding rows gets the earlier entry depends
 * on arrival; what rg_rx_table_find and the kernels' lookup answer does not.  Probing is bounded by rx_cap.
 *
 * The wrappers take the handshake calls' outputs as they are, through the same kernels:
 *   rg_session_install_resp_batch_dev    local id session_ids[i], remote id results[i].sender, peer
 *                                        results[i].peer, keys rg_handshake_resp_batch_dev's transport_keys
 *   rg_session_install_finish_batch_dev  local id pend_session_ids[pend_idx_out[i]], peer
 *                                        pend_peers[pend_idx_out[i]], remote id remote_out[i], keys
 *                                        rg_handshake_finish_batch_dev's transport_keys; pend_session_ids and
 *                                        pend_peers are the session_ids and peer_idx the initiate call was given;
 *                                        pend_idx_out[i] >= npending on a row whose gate is OK: RG_PKT_INVALID
 * gate is the status array of the call whose outputs they take.
 *
 * rg_session_expire_batch_dev: one lane per row.  A live row r leaves if now_ns and
 * send_state[r].started_ns + 180e9 < *now_ns (u64 wrapping add, strict <: rg_send_reserve_batch_dev's rule,
 * should_expire), or if rows[m] names it (rg_sessions_remove; entries >= nkeys are ignored).  Its two keys,
 * window and send state are zeroed, receivers[r] = local_ids[r] = 0, peer_slot[p] = RG_KEY_SKIP only if it still
 * names r (time.rs:93-95), slot_peer[r] = RG_PEER_NONE.  expired_out[nkeys] (may be NULL) gets 1 for a row that
 * left and 0 for every other.  Then rx_table is rebuilt.
 *
 * rg_session_index_dev is that rebuild alone. */
size_t rg_session_workspace_size(size_t n, uint32_t nkeys, uint32_t npeers);
int rg_session_install_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint8_t *gate /* [n] or NULL */,
                                 const uint32_t *local_ids /* [n] */, const uint32_t *remote_ids /* [n] */,
                                 const uint32_t *peers /* [n] */, uint8_t *transport_keys /* [n][64], zeroed */,
                                 size_t n, const uint64_t *now_ns, uint8_t *status /* [n] */,
                                 uint32_t *rows_out /* [n] */, void *workspace, size_t workspace_len, void *stream);
int rg_session_install_resp_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint8_t *gate,
                                      const uint32_t *session_ids /* [n] */, const rg_hs_init_result *results,
                                      uint8_t *transport_keys, size_t n, const uint64_t *now_ns, uint8_t *status,
                                      uint32_t *rows_out, void *workspace, size_t workspace_len, void *stream);
int rg_session_install_finish_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint8_t *gate,
                                        const uint32_t *pend_idx_out /* [n] */, const uint32_t *remote_out /* [n] */,
                                        const uint32_t *pend_session_ids /* [npending] */,
                                        const uint32_t *pend_peers /* [npending] */, uint32_t npending,
                                        uint8_t *transport_keys, size_t n, const uint64_t *now_ns, uint8_t *status,
                                        uint32_t *rows_out, void *workspace, size_t workspace_len, void *stream);
int rg_session_expire_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint64_t *now_ns /* or NULL */,
                                const uint32_t *rows /* [m] or NULL */, size_t m,
                                uint8_t *expired_out /* [nkeys] or NULL */, void *workspace, size_t workspace_len,
                                void *stream);
int rg_session_index_dev(rg_ctx *ctx, const rg_session_tables *tables, void *stream);

/* ------------------------------ device-resident session timers (batch, async) */
/* What Sessions::turn (rustyguard-core/src/time.rs:42-140, tick_timers) decides for transport sessions, on the
 * stream that sends and receives: which sessions owe a keepalive and which peers owe a new handshake, as the
 * arrays rg_send_batch_dev_resident and the initiator chain take.  Expiry stays rg_session_expire_batch_dev, run
 * behind the turn.  The handshake-side timers (InitAttempt, ExpireHandshake, current_handshake) are the next
 * section's, whose turn takes this turn's rekey list.
 *
 * The conventions are the session-table section's: every array is device memory; the calls enqueue on `stream`
 * and return without waiting, allocate nothing and keep nothing in the context (so they can be captured into a
 * graph); now_ns points at one uint64_t in device memory, read when the kernels run; n == 0 returns RG_OK;
 * RG_EINVAL with nothing enqueued for a null required pointer (gate is optional, now_ns of the arm call when
 * rekey_after_ns == 0, timers and send_state when nkeys == 0, the three lists when npeers == 0), n > 2^32 - 1, a
 * misaligned array (timers, send_state, now_ns 8 bytes, word arrays 4, the workspace 16) or a workspace smaller
 * than rg_timer_workspace_size(nkeys, npeers) reports (0 when either size is above 2^32 - 1; non-decreasing in
 * each argument).  The workspace belongs to one call at a time.  A lane stores its output after everything else
 * it writes.  All time arithmetic is the u64 wrapping add and strict < of rg_send_reserve_batch_dev.
 *
 * One rg_session_timer row runs parallel to every key-table row; the caller owns the array, and a zeroed row has
 * nothing armed.  It holds what the reference's timer heap holds for a transport session. */
#define RG_TIMER_KEEPALIVE_PENDING 1u /* Session.keepalive_pending */
typedef struct rg_session_timer {    /* 16 bytes, 8-byte aligned */
    uint64_t rekey_at_ns;            /* the RekeyAttempt heap entry: 0 = not armed, fires when rekey_at_ns < now */
    uint32_t flags;                  /* RG_TIMER_KEEPALIVE_PENDING */
    uint32_t pad;
} rg_session_timer;

/* rg_timer_arm_batch_dev runs behind an install, on its rows_out and status (as gate; NULL: every row passes): for
 * every i with gate[i] == RG_PKT_OK and rows[i] < nkeys,
 *   timers[rows[i]] = { rekey_after_ns ? *now_ns + rekey_after_ns : 0, 0, 0 }.
 * rekey_after_ns is a host scalar: RG_REKEY_AFTER_TIME_NS for sessions we initiated (handshake.rs:218-222), 0 for
 * sessions we responded to, where the reference arms no rekey.  Every install is followed by an arm: that is also
 * what clears the stale row of a session that expired.
 *
 * rg_timer_note_send_batch_dev runs behind rg_send_batch_dev_resident or rg_send_batch_dev_routed, on their slots
 * (for the routed send the slots at the head of its workspace's descriptors), status and rekey_out
 * (lib.rs:564-570): for every i with status[i] == RG_PKT_OK, rekey_out[i] != 0 and slots[i] < nkeys, a
 * rekey_at_ns that is 0 or greater than *now_ns becomes *now_ns.  Every lane that writes a row writes the same
 * value.  A clock of 0 arms nothing (0 is "not armed").
 *
 * rg_timer_note_recv_batch_dev runs behind rg_recv_batch_dev_resident, on its key_idx_out and status, ahead of or
 * beside rg_route_check_batch_dev (lib.rs:664-669; the reference, too, flags the keepalive before handle_extern):
 * for every i with status[i] == RG_PKT_OK and k = key_idx[i] < nkeys, if
 * send_state[k].sent_ns + RG_KEEPALIVE_TIMEOUT_NS < *now_ns the row's RG_TIMER_KEEPALIVE_PENDING is set (atomicOr).
 *
 * rg_timer_turn_dev is tick_timers for the whole table in one pass.  Of the tables it reads slot_peer, send_state,
 * peer_slot, nkeys and npeers and writes none.  Its result equals this loop, bit for bit on every byte of timers,
 * on ka_slots_out, rekey_peers_out and rekey_gate_out over their full npeers entries and on counts_out; every
 * decision reads the state as it stands before the call:
 *   now = *now_ns;  want_ka[p] = want_rk[p] = 0
 *   for r in 0..nkeys with p = slot_peer[r] != RG_PEER_NONE and p < npeers:        (free rows are not touched)
 *     if timers[r].flags & RG_TIMER_KEEPALIVE_PENDING:                              (time.rs:114-125)
 *       clear it;  if send_state[r].sent_ns + 10e9 < now: want_ka[p] = 1
 *     if timers[r].rekey_at_ns != 0 and timers[r].rekey_at_ns < now:                (time.rs:49-66; popped)
 *       timers[r].rekey_at_ns = 0
 *       if send_state[r].started_ns + 120e9 < now
 *          or send_state[r].counter >= RG_REKEY_AFTER_MESSAGES: want_rk[p] = 1
 *   nka = nrk = 0
 *   for p ascending:
 *     c = peer_slot[p]
 *     if want_ka[p] and c < nkeys and slot_peer[c] == p                             (encrypt_message,
 *        and not (send_state[c].started_ns + 180e9 < now                             lib.rs:249-265: the peer's
 *                 or send_state[c].counter >= RG_REJECT_AFTER_MESSAGES):             CURRENT row, should_reject)
 *       ka_slots_out[nka++] = c
 *     if want_rk[p]: rekey_peers_out[nrk++] = p
 *   ka_slots_out[nka..npeers) = RG_KEY_SKIP;  rekey_peers_out[nrk..npeers) = RG_PEER_NONE
 *   rekey_gate_out[k] = RG_PKT_OK for k < nrk, RG_PKT_REJECTED above;  counts_out = {nka, nrk}
 * computed with one lane per row, one lane per peer and an exclusive count over the peers; want_ka / want_rk get
 * the same value from every row of a peer.  The padding lets the next calls run with the host-side n = npeers and
 * no read-back: ka_slots_out is the slots of rg_send_batch_dev_resident over a fixed descriptor array of 32-byte
 * frames with len = 0 (RG_KEY_SKIP rows are RG_PKT_REJECTED there, no counter taken, frame untouched; the send
 * stores sent_ns = now); rekey_peers_out and rekey_gate_out are the peer_idx and gate of
 * rg_handshake_initiate_batch_dev and rg_peer_mac1_batch_dev.
 *
 * Unlike the reference: a peer gets at most one keepalive a turn, decided on the state before the turn (the
 * reference pops entries in time order, ties arbitrary, so two pending sessions of one peer yield one keepalive or
 * two); a row holds one RekeyAttempt entry (the reference pushes one per send past REKEY_AFTER_MESSAGES);
 * endpoints are the peer-endpoint section's: rg_endpoint_gate_batch_dev on ka_slots_out, rg_endpoint_peers_batch_dev
 * on rekey_peers_out. */
size_t rg_timer_workspace_size(size_t nkeys, size_t npeers);
int rg_timer_arm_batch_dev(rg_ctx *ctx, rg_session_timer *timers, uint32_t nkeys, const uint32_t *rows /* [n] */,
                           const uint8_t *gate /* [n] or NULL */, size_t n, const uint64_t *now_ns,
                           uint64_t rekey_after_ns, void *stream);
int rg_timer_note_send_batch_dev(rg_ctx *ctx, rg_session_timer *timers, uint32_t nkeys, const uint32_t *slots /* [n] */,
                                 const uint8_t *status /* [n] */, const uint8_t *rekey_out /* [n] */, size_t n,
                                 const uint64_t *now_ns, void *stream);
int rg_timer_note_recv_batch_dev(rg_ctx *ctx, rg_session_timer *timers, const rg_send_state *send_state,
                                 uint32_t nkeys, const uint32_t *key_idx /* [n] */, const uint8_t *status /* [n] */,
                                 size_t n, const uint64_t *now_ns, void *stream);
int rg_timer_turn_dev(rg_ctx *ctx, const rg_session_tables *tables, rg_session_timer *timers, const uint64_t *now_ns,
                      uint32_t *ka_slots_out /* [npeers] */, uint32_t *rekey_peers_out /* [npeers] */,
                      uint8_t *rekey_gate_out /* [npeers] */, uint32_t counts_out[2], void *workspace,
                      size_t workspace_len, void *stream);

/* ------------------------------ device-resident pending handshakes (batch, async) */
/* The initiator's side of Sessions between "this peer needs a handshake" and "its response arrived", on the
 * stream that sends and receives: the pending-handshake table with Peer.current_handshake, and the two
 * handshake-side timers, InitAttempt and ExpireHandshake (rustyguard-core/src/time.rs:49-83, 99-113; armed in
 * handshake.rs:260-325).  Three calls on a running tunnel name peers that need a handshake -- rg_timer_turn_dev's
 * rekey list, the routed send's RG_PKT_REJECTED rows with their peers_out, and an initiation that got no answer
 * for REKEY_TIMEOUT -- and rg_pending_turn_dev merges all three into the one list the initiator chain takes;
 * rg_pending_install_batch_dev puts the chain's pending rows into the table rg_handshake_finish_batch_dev reads.
 * No host read lies between a lost packet and its retry.
 *
 * The conventions are the session-table and timer sections': every array is device memory; the calls enqueue on
 * `stream` and return without waiting, allocate nothing and keep nothing in the context (so they can be captured
 * into a graph; every fill is a kernel, no memset node); now_ns points at one uint64_t in device memory, read when
 * the kernels run; n == 0 returns RG_OK; RG_EINVAL with nothing enqueued -- and before the device is touched at
 * all -- for a null required pointer (gate, expired_out and start_status are optional, start_peers when m == 0, the
 * three per-peer table arrays when npeers == 0), a count above 2^32 - 1, a misaligned array (struct rows 16 bytes;
 * rg_pending_timer rows, pend_table and now_ns 8; word arrays 4; the workspace 16), pend_cap not a power of two
 * or < 2 npeers, or a workspace smaller than rg_pending_workspace_size(n, m, npeers) reports (0 when a size is
 * above 2^32 - 1; non-decreasing in each argument; the install is asked with m = 0, the turn with n = 0).  The
 * workspace belongs to one call at a time.  A lane stores its status after everything else it writes.  All time
 * arithmetic is the u64 wrapping add and strict < of rg_send_reserve_batch_dev.  Nothing is decided by the order
 * the lanes arrive in.
 *
 * The table is indexed by peer: current_handshake holds at most one pending handshake a peer.  The caller owns
 * the arrays and passes them in a host struct that is read at call time.  An empty table has `pending` zeroed with
 * peer = RG_PEER_NONE, pend_table 0xFF and the rest zero.  Liveness has one source, pending[p].peer == p: the
 * finish call's wipe of a row ends its life with no further call, and a stale pend_table entry that names a
 * wiped row is harmless (the finish call answers RG_PKT_REJECTED).  rg_handshake_finish_batch_dev is used with
 * pending = tables.pending and npending = npeers, so its pend_idx_out is the peer;
 * rg_session_install_finish_batch_dev with pend_session_ids = hs_ids and pend_peers = the caller's constant array
 * 0..npeers-1. */
#define RG_REKEY_TIMEOUT_NS       5000000000ull   /* REKEY_TIMEOUT, lib.rs:69 */
#define RG_REKEY_ATTEMPT_TIME_NS 90000000000ull   /* REKEY_ATTEMPT_TIME, lib.rs:68 */
typedef struct rg_pending_timer {    /* 16 bytes, 8-byte aligned: Session.started / .sent of a handshake */
    uint64_t started_ns;             /* the first attempt of this run of retries */
    uint64_t sent_ns;                /* the latest attempt */
} rg_pending_timer;
typedef struct rg_pending_tables {
    rg_hs_pending    *pending;    /* [npeers]   row p is peer p's current_handshake; live iff pending[p].peer == p */
    rg_pending_timer *timers;     /* [npeers]   meaningful for live rows only                                     */
    uint32_t         *hs_ids;     /* [npeers]   sender id of the last handshake installed for p; survives the     */
                                  /*            finish call's wipe                                                */
    rg_rx_entry      *pend_table; /* [pend_cap] receiver id -> p over the live rows; pend_cap a power of two      */
                                  /*            >= 2 npeers                                                       */
    uint32_t npeers, pend_cap;
} rg_pending_tables;

/* rg_pending_index_dev rebuilds pend_table from the live rows: a fill with 0xFF, then one lane per live row claims
 * the first empty entry from its id's home slot (the receiver-table rebuild's method).  Probing is bounded by
 * pend_cap, and no index leaves the table.
 *
 * rg_pending_install_batch_dev is the tail of new_handshake (handshake.rs:266-297), run behind
 * rg_handshake_initiate_batch_dev on its pending[n] output (`batch`) and its status (`gate`).  Its result equals
 * this loop, bit for bit on status, installed_out, every byte of batch, tables.pending, timers and hs_ids, and on
 * pend_table through its lookup:
 *   now = *now_ns;  live0[p] = (pending[p].peer == p) before the call
 *   for i in array order:
 *     installed_out[i] = RG_PEER_NONE
 *     gate && gate[i] != RG_PKT_OK -> status RG_PKT_REJECTED; nothing else of row i read or written
 *     row = batch[i]; batch[i] = zeros with peer = RG_PEER_NONE    (a pending row is consumed once, whatever follows)
 *     p = row.peer;  p >= npeers -> RG_PKT_INVALID
 *     status RG_PKT_OK
 *     the LAST such i of a peer p in array order is stored:        (each new_handshake replaces the one before)
 *       pending[p] = row; hs_ids[p] = row.sender
 *       timers[p] = { live0[p] ? timers[p].started_ns : now, now } (handshake.rs:281-293: a retry keeps `started`)
 *       installed_out[i] = p
 *   pend_table = the table over the live rows
 * computed with atomicMax(claim[p], i + 1), a commit over the peers that moves the 128-byte row in 16-byte pieces,
 * and a wipe over the batch that runs after the commit has read it.  batch must not overlap tables.pending
 * (RG_EINVAL).  Sender ids are the caller's and must be unique among live rows; with a repeat the call stays
 * memory-safe, and which row the lookup answers is unspecified.
 *
 * rg_pending_turn_dev is the InitAttempt and ExpireHandshake arms of tick_timers for the whole table, and the
 * merge of every other source of "this peer needs a handshake" into one list, so that a turn costs one initiate
 * call whatever the number of sources.  start_peers[m] / start_status[m] / start_match is a request list: entry j
 * counts iff start_status == NULL or start_status[j] == start_match.  That fits rg_timer_turn_dev's
 * rekey_peers_out / rekey_gate_out with RG_PKT_OK and the routed send's peers_out / status with RG_PKT_REJECTED;
 * the call is made once per source, or once on a concatenation the caller keeps.  Its result equals this loop, bit
 * for bit on every byte of tables.pending and timers, on the three output arrays over their full npeers and on
 * counts_out:
 *   now = *now_ns; want[p] = 0; nexp = 0
 *   for p in 0..npeers with pending[p].peer == p:
 *     timers[p].sent_ns + 90e9 < now     -> pending[p] = zeros, peer = RG_PEER_NONE; timers[p] = 0;
 *                                           expired_out[p] = 1; nexp++       (time.rs:99-113; armed at the attempt's
 *                                                                             now + REKEY_ATTEMPT_TIME, handshake.rs:319-322)
 *     else sent_ns + 5e9 < now and now < started_ns + 90e9
 *                                        -> want[p] = 1; timers[p].sent_ns = now  (should_reinit, lib.rs:194-196;
 *                                                                                  new_handshake stamps `sent` before it can fail)
 *   expired_out[p] = 0 for every other p (expired_out may be NULL)
 *   for j in 0..m that counts, q = start_peers[j] < npeers:
 *     pending[q].peer != q (after the loop above) -> want[q] = 1
 *   for p ascending with want[p]: init_peers_out[k++] = p
 *   init_peers_out[k..npeers) = RG_PEER_NONE; init_gate_out = RG_PKT_OK below k, RG_PKT_REJECTED above
 *   counts_out = {k, nexp};  pend_table = the table over the live rows (rebuilt on every call)
 * computed with a clear kernel, one lane per peer, one lane per request and an exclusive count over the peers, both
 * counts in one 64-bit sum.  hs_ids is written by the install only.  The two row rules cannot both hold without
 * clock wrap: started_ns <= sent_ns, so sent_ns + 90e9 < now implies started_ns + 90e9 < now, and the second rule
 * asks for the opposite; with a clock that wraps between them the expiry is taken, as the order above says.
 * init_peers_out / init_gate_out are the peer_idx / gate of rg_peer_cookies_batch_dev ->
 * rg_handshake_initiate_batch_dev -> rg_peer_mac1_batch_dev -> rg_pending_install_batch_dev, each run with the
 * host-side n = npeers.
 *
 * Unlike the reference: (a) it starts a new handshake for every sessionless packet and every fired rekey, replacing
 * one in flight (lib.rs:575-580); here a request for a peer with a live pending row is dropped and the row's own
 * 5 s retry governs -- otherwise a batch of packets a millisecond later would replace the handshake before its
 * response can arrive.  (b) The timers are evaluated statelessly on {started_ns, sent_ns}, not popped from a heap;
 * the same entries fire: InitAttempt at sent + 5 s, ExpireHandshake at sent + 90 s, and no retry once
 * now >= started + 90 s.  (c) Session ids, esk and timestamps stay the caller's;
 * endpoints are the peer-endpoint section's (rg_endpoint_peers_batch_dev on init_peers_out). */
size_t rg_pending_workspace_size(size_t n, size_t m, uint32_t npeers);
int rg_pending_index_dev(rg_ctx *ctx, const rg_pending_tables *tables, void *stream);
int rg_pending_install_batch_dev(rg_ctx *ctx, const rg_pending_tables *tables, rg_hs_pending *batch /* [n] */,
                                 const uint8_t *gate /* [n] or NULL */, size_t n, const uint64_t *now_ns,
                                 uint8_t *status /* [n] */, uint32_t *installed_out /* [n] */, void *workspace,
                                 size_t workspace_len, void *stream);
int rg_pending_turn_dev(rg_ctx *ctx, const rg_pending_tables *tables, const uint64_t *now_ns,
                        const uint32_t *start_peers /* [m] or NULL */, const uint8_t *start_status /* [m] or NULL */,
                        uint8_t start_match, size_t m, uint32_t *init_peers_out /* [npeers] */,
                        uint8_t *init_gate_out /* [npeers] */, uint8_t *expired_out /* [npeers] or NULL */,
                        uint32_t counts_out[2], void *workspace, size_t workspace_len, void *stream);

/* ------------------------------ device-resident handshake rate limiter (batch, async) */
/* DynamicState::overloaded (rustyguard-core/src/lib.rs:508-514) on the stream that runs the responder chain: the
 * count-min sketch over source addresses (rustyguard-utils/src/rate_limiter.rs, CountMinSketch::with_params(10.0 /
 * 20_000.0, 0.01, rng)) that handle_handshake_init and handle_handshake_resp bump once per handshake message before
 * the MACs are looked at (handshake.rs:47, :151), and Sessions::turn's wipe and reseed (lib.rs:406-408).
 * rg_rate_count_batch_dev's overload_out is the `overload` argument of rg_cookie_reply_batch_dev on the same
 * stream, so the filter's last input needs no host step: rg_rate_turn_dev -> rg_rate_count_batch_dev ->
 * rg_cookie_reply_batch_dev -> the responder chain.
 *
 * The conventions are the session-table, timer and pending sections': every array is device memory unless marked
 * host; the calls enqueue on `stream` and return without waiting, allocate nothing and keep nothing in the context
 * (so they can be captured into a graph; every fill is a kernel, no memset node); now_ns points at one uint64_t in
 * device memory, read when the kernels run; n == 0 returns RG_OK; RG_EINVAL with nothing enqueued -- and before the
 * device is touched at all -- for a null required pointer (counts_out is optional), a count above 2^32 - 1 (n,
 * n * depth, and width * depth, the number of buckets), a misaligned array (seeds, new_seeds and the workspace 16
 * bytes; rg_src_addr rows, now_ns and last_reset_ns 8; word arrays 4), depth == 0, depth > RG_RATE_MAX_DEPTH,
 * width == 0, or a workspace smaller than rg_rate_workspace_size(n, width, depth) reports (0 when a size is out of
 * range; non-decreasing in each argument within it).  The workspace belongs to one call at a time.  Nothing is
 * decided by the order the lanes arrive in: no atomic's return value is used.
 *
 * The caller owns the arrays and passes them in a host struct that is read at call time.  An empty sketch is all
 * zero.  width and depth are free (a test can force collisions with a tiny sketch); the defaults are the
 * reference's.
 *
 * Key of a source address (lib.rs:509-512): an address whose ip[4..16] is all zero is IPv4 and key = the big-endian
 * u32 of ip[0..4]; any other address is keyed by its /64, key = the big-endian u64 of ip[0..8].  The port is
 * ignored.
 * Column of key in sketch row r:
 *   fold(x, y) = the low 64 bits XOR the high 64 bits of the 128-bit product x * y
 *   h   = fold(fold(key ^ seeds[r].a, 0x9E3779B97F4A7C15) ^ seeds[r].b, 0xD6E8FEB86659FD93)
 *   col = (uint32_t)(((h >> 32) * width) >> 32)
 * rg_rate_column is that column for one address and one seed, computed on the host from the code the kernels
 * compile (NULL seed or addr: 0).
 *
 * rg_rate_count_batch_dev takes the desc and buf of rg_cookie_reply_batch_dev and never writes buf.  A message is
 * counted exactly when the filter would go on to read its MACs: offset % 16 == 0, the frame inside [buf, buf +
 * buf_len), len == 148 with type word 1 or len == 92 with type word 2, and key_idx != RG_KEY_SKIP.  Its result
 * equals this loop, bit for bit on counts_out (may be NULL), overload_out and every bucket:
 *   for i in array order:
 *     not counted -> counts_out[i] = 0; overload_out[i] = 0
 *     else est = 0xFFFFFFFF
 *          for r in 0..depth: c = col_r(key(addrs[i])); b = buckets[r][c] = sat_add_u32(buckets[r][c], 1)
 *                             est = min(est, b)
 *          counts_out[i] = est; overload_out[i] = est > limit
 * computed over the n * depth items (message, sketch row): one stable grouping by the bucket r * width + col (two
 * 8-bit radix passes at the default size), a segmented inclusive count of the counted items, estimate =
 * sat_add(bucket, rank); the last item of each bucket's group stores the bucket, and one lane per message takes the
 * minimum over its depth items and stores overload_out last.
 *
 * rg_rate_turn_dev:
 *   now = *now_ns; last = *last_reset_ns
 *   now > last and now - last > period_ns -> buckets = 0; seeds = new_seeds; *last_reset_ns = now; *reset_out = 1
 *   else                                  -> *reset_out = 0; nothing else written
 * One lane decides and writes reset_out and last_reset_ns; the wipe behind it reads reset_out alone, so a replayed
 * graph reads its clock when it runs.  Randomness: the library has no RNG.  new_seeds is depth fresh 16-byte
 * outputs of the caller's CSPRNG, refreshed every turn like the cookie nonces and consumed only on a reset.
 *
 * Unlike the reference: (a) the hash.  The reference hashes with foldhash under random seeds that are redrawn every
 * second; no output of that hash is observable or reproducible, and its source is not available to this project.
 * What is kept is the contract: a keyed 64-bit hash per sketch row, seeded from the caller's RNG.  (b) The reference
 * never assigns last_rate_reset (lib.rs:361, 376 and 406 are its only uses), so it wipes on every turn in which the
 * clock advanced; period_ns = 0 reproduces exactly that, and RG_RATE_PERIOD_NS gives the one-second window the
 * comparison was written for. */
#define RG_RATE_WIDTH      5437u           /* ceil(e / (10/20000)), rate_limiter.rs:54-60 with lib.rs:377 */
#define RG_RATE_DEPTH      5u              /* ceil(ln(1/0.01)) */
#define RG_RATE_LIMIT      10u             /* overloaded: count > 10, lib.rs:513 */
#define RG_RATE_MAX_DEPTH  8u
#define RG_RATE_PERIOD_NS  1000000000ull   /* lib.rs:406 */
typedef struct rg_rate_seed { uint64_t a, b; } rg_rate_seed;   /* 16 bytes; the caller's CSPRNG output */
typedef struct rg_rate_tables {            /* host struct, read at call time */
    uint32_t     *buckets;        /* [depth][width], row-major; an empty sketch is all zero */
    rg_rate_seed *seeds;          /* [depth] */
    uint64_t     *last_reset_ns;  /* [1], starts 0 */
    uint32_t width, depth;
} rg_rate_tables;

uint32_t rg_rate_column(const rg_rate_seed *seed /* host */, const rg_src_addr *addr /* host */, uint32_t width);
size_t rg_rate_workspace_size(size_t n, uint32_t width, uint32_t depth);
int rg_rate_count_batch_dev(rg_ctx *ctx, const rg_rate_tables *tables, const rg_pkt_desc *desc,
                            const rg_src_addr *addrs, size_t n, const uint8_t *buf, size_t buf_len, uint32_t limit,
                            uint32_t *counts_out /* [n] or NULL */, uint8_t *overload_out /* [n] */,
                            void *workspace, size_t workspace_len, void *stream);
int rg_rate_turn_dev(rg_ctx *ctx, const rg_rate_tables *tables, const uint64_t *now_ns, uint64_t period_ns,
                     const rg_rate_seed *new_seeds /* [depth], caller's CSPRNG */, uint32_t *reset_out /* [1] */,
                     void *stream);

/* ------------------------------ device-resident peer endpoints (batch, async) */
/* PeerState.endpoint (rustyguard-core/src/lib.rs:160-181) on the stream that sends and receives: where each peer's
 * packets last came from, moved only by what was authenticated, and handed to the next send as a destination array.
 * The reference moves it in decrypt_packet for every data packet that is authenticated and passes anti-replay
 * (lib.rs:659-671; keepalives count, a forged or replayed packet does not -- its test
 * forged_packet_does_not_update_peer_endpoint) and in handle_handshake_resp for the response that finishes a pending
 * handshake (handshake.rs:205); handle_handshake_init does not touch it.  It reads it in send_message (lib.rs:550-553:
 * a peer without one is Error::Rejected before anything is encrypted) and for keepalives and rekey initiations
 * (time.rs:67, :135).  With these calls receive -> note -> ... -> gate -> send is one chain with no host read, and the
 * output of a turn is frames plus a destination address array.
 *
 * The conventions are the peer-state and session sections': every pointer is device memory; the calls enqueue on
 * `stream` and return without waiting, allocate nothing and keep nothing in the context (so they can be captured
 * into a graph; no memset node); n == 0 returns RG_OK; RG_EINVAL with nothing enqueued -- and before the device is
 * touched at all -- for a null pointer (every array is required), n > 2^32 - 1 or a misaligned array (endpoints 16
 * bytes; rg_src_addr rows 8; word arrays 4).  A lane stores what it decides after everything else it writes.  No
 * index reaches memory unchecked.  Nothing is decided by the order the lanes arrive in.
 *
 * One rg_endpoint row runs parallel to every rg_hs_peer row; the caller owns the array.  A zeroed row is None, and
 * the configured endpoint of a peer (PeerState::new(p.endpoint)) is stored by the caller before the first call.  A
 * row counts as Some when `set` is not 0.  Addresses come in and go out as rg_src_addr, of which the first 18 bytes
 * are meaningful; every rg_src_addr these calls write has `pad` zero, so the same arrays feed the filter and the rate
 * limiter. */
typedef struct rg_endpoint {         /* 32 bytes, rows 16-byte aligned; zeroed = None */
    uint8_t  ip[16];                 /* rg_src_addr's encoding */
    uint16_t port_le;
    uint16_t set;                    /* 0 = None, 1 = Some; nothing else is ever written */
    uint8_t  zero[12];               /* always written as zero */
} rg_endpoint;

/* The three note calls change the table.  Each equals this loop, bit for bit on every byte of endpoints:
 *   for i in array order:
 *     status[i] == RG_PKT_OK and p = peer_of(i) < npeers -> endpoints[p] = { src[i].ip, src[i].port_le, 1, zeros }
 * and every other row keeps its bytes.  They differ in peer_of alone:
 *   rg_endpoint_note_recv_batch_dev    runs behind rg_recv_batch_dev_resident on its key_idx_out and status and IN FRONT
 *                                      OF rg_route_check_batch_dev (the reference has moved the endpoint before the
 *                                      source check, and the check overwrites RG_PKT_OK):
 *                                      peer_of(i) = slot_peer[key_idx[i]] when key_idx[i] < nkeys, none otherwise; a
 *                                      free row (RG_PEER_NONE) names no peer
 *   rg_endpoint_note_peers_batch_dev   peer_of(i) = peer_idx[i]
 *   rg_endpoint_note_finish_batch_dev  runs behind rg_handshake_finish_batch_dev on its pend_idx_out and status:
 *                                      peer_of(i) = pend_peers[pend_idx_out[i]] when pend_idx_out[i] < npending
 * computed with atomicMax(claim[p], i + 1) -- reduced within each wave first, so a batch of one session costs one
 * atomic a wave -- and a commit in which the lane whose i + 1 is the claim stores the row and then puts the claim
 * word back to 0.  claim is npeers words the caller zeroes ONCE; every call leaves it zeroed, no fill is enqueued and
 * the cost follows n, not npeers.  A claim array that is not zero makes the call skip peers; it stays memory-safe (the
 * claim word is compared, never used as an index).  claim belongs to one call at a time.
 *
 * The two gather calls only read the table, one lane per item:
 *   rg_endpoint_gate_batch_dev   runs in front of rg_send_batch_dev_resident, behind rg_route_batch_dev or on
 *                                rg_timer_turn_dev's ka_slots_out.  If slots[i] < nkeys, p = slot_peer[slots[i]] <
 *                                npeers and endpoints[p] is Some: slots_out[i] = slots[i], dst_out[i] = the address
 *                                with pad zero.  Otherwise slots_out[i] = RG_KEY_SKIP and dst_out[i] is 24 zero bytes;
 *                                the send then reports RG_PKT_REJECTED, takes no counter and leaves the frame alone,
 *                                which is send_message's early return.  slots_out may be slots.
 *   rg_endpoint_peers_batch_dev  the same by peer with RG_PEER_NONE as the "no" value, for the rekey and pending
 *                                lists that feed rg_peer_cookies_batch_dev -> rg_handshake_initiate_batch_dev ->
 *                                rg_peer_mac1_batch_dev, which take a RG_PEER_NONE row as it is.  peers_out may be
 *                                peer_idx.
 *
 * Unlike the reference: (a) a keepalive or rekey for a peer without an endpoint is skipped, where time.rs:67 and :135
 * `expect` one; (b) the claim and commit replace arrival order: the last eligible item in ARRAY order wins, which is
 * the in-order loop's result whatever order the lanes run in. */
int rg_endpoint_note_recv_batch_dev(rg_ctx *ctx, rg_endpoint *endpoints, uint32_t npeers,
                                    const uint32_t *slot_peer /* [nkeys] */, uint32_t nkeys,
                                    const uint32_t *key_idx /* [n] */, const uint8_t *status /* [n] */,
                                    const rg_src_addr *src /* [n] */, size_t n, uint32_t *claim /* [npeers] */,
                                    void *stream);
int rg_endpoint_note_peers_batch_dev(rg_ctx *ctx, rg_endpoint *endpoints, uint32_t npeers,
                                     const uint32_t *peer_idx /* [n] */, const uint8_t *status /* [n] */,
                                     const rg_src_addr *src /* [n] */, size_t n, uint32_t *claim /* [npeers] */,
                                     void *stream);
int rg_endpoint_note_finish_batch_dev(rg_ctx *ctx, rg_endpoint *endpoints, uint32_t npeers,
                                      const uint32_t *pend_idx_out /* [n] */, const uint32_t *pend_peers /* [npending] */,
                                      uint32_t npending, const uint8_t *status /* [n] */,
                                      const rg_src_addr *src /* [n] */, size_t n, uint32_t *claim /* [npeers] */,
                                      void *stream);
int rg_endpoint_gate_batch_dev(rg_ctx *ctx, const rg_endpoint *endpoints, uint32_t npeers,
                               const uint32_t *slot_peer /* [nkeys] */, uint32_t nkeys, const uint32_t *slots /* [n] */,
                               size_t n, uint32_t *slots_out /* [n] */, rg_src_addr *dst_out /* [n] */, void *stream);
int rg_endpoint_peers_batch_dev(rg_ctx *ctx, const rg_endpoint *endpoints, uint32_t npeers,
                                const uint32_t *peer_idx /* [n] */, size_t n, uint32_t *peers_out /* [n] */,
                                rg_src_addr *dst_out /* [n] */, void *stream);

/* ------------------------------ device-resident inbound demultiplexer (batch, async) */
/* The `match msg_type` of Sessions::recv_message (rustyguard-core/src/lib.rs:605-630) on the stream that runs the
 * chains behind it: one array of datagrams in arrival order -- what recvmmsg hands a node, message types 1-4 and junk
 * interleaved -- is split into the descriptor lists the existing calls take as they are, and the chains' verdicts are
 * carried back to the datagrams' own order.  With these two calls a mixed batch goes from one descriptor array to its
 * final per-datagram statuses with no host read in between:
 *   rg_demux_batch_dev -> handshake list: rg_rate_count_batch_dev -> rg_cookie_reply_batch_dev (over hs_desc, hs_addrs)
 *                                         -> rg_handshake_init_batch_dev (over init_desc, gate = the filter's status)
 *                                         -> rg_handshake_finish_batch_dev (over resp_desc, the same gate)
 *                      -> cookie list:    rg_peer_cookie_consume_batch_dev (over ck_desc)
 *                      -> data list:      rg_recv_batch_dev_resident -> rg_endpoint_note_recv_batch_dev (data_addrs)
 *   -> rg_demux_verdict_batch_dev
 *
 * The conventions are the peer-state, session and endpoint sections': every array is device memory; the calls enqueue
 * on `stream` and return without waiting, allocate nothing and keep nothing in the context (so they can be captured
 * into a graph; every fill is a kernel, no memset node); every scratch array lives in `workspace`, 16-byte aligned
 * and at least rg_demux_workspace_size(n) bytes (0 for n > 2^32 - 1), which belongs to one call at a time; n == 0
 * returns RG_OK with nothing written; RG_EINVAL with nothing enqueued -- and before the device is touched at all --
 * for a null required pointer (the arrays of a list whose capacity is 0 may be NULL), n > 2^32 - 1, a misaligned
 * array (rg_pkt_desc rows and the workspace 16 bytes; rg_src_addr rows 8; buf, pos and counts 4) or a short workspace.
 * Nothing is decided by the order the lanes arrive in: there is no atomic.  buf is never written.  A lane stores
 * status[i] after everything else it writes.  No index reaches memory unchecked.
 *
 * Three lists, because that is how the existing calls consume them.  The handshake list holds types 1 and 2 together
 * in array order: rg_rate_count_batch_dev and rg_cookie_reply_batch_dev both take mixed 148 / 92-byte messages, and the
 * sketch's result depends on the array order of every handshake message of a source (the reference calls overloaded()
 * in handle_handshake_init and handle_handshake_resp alike, handshake.rs:47, :151).  It is four parallel arrays of
 * cap_hs rows: hs_desc, every listed message; hs_addrs, their source addresses with `pad` zeroed; init_desc, row k =
 * hs_desc[k] if the message is type 1, else the inert row; resp_desc, the same for type 2.  Because the four are
 * parallel, the filter's status array over hs_desc is, unchanged, the `gate` of rg_handshake_init_batch_dev over
 * init_desc and of rg_handshake_finish_batch_dev over resp_desc.
 *
 * The inert row is { offset 0, len 0, RG_KEY_SKIP }, with 24 zero bytes for an address row, and every row of every
 * list beyond its count is the inert row, so a replayed graph never sees stale rows.  Every consumer turns it away on
 * its length rule, which it applies before it reads buf (offset 0 is aligned and a frame of 0 bytes is inside any buf):
 *   rg_cookie_reply_batch_dev, rg_rate_count_batch_dev  len is neither 148 nor 92: RG_PKT_INVALID / not counted
 *   rg_handshake_init_batch_dev                         len is not 148: RG_PKT_INVALID
 *   rg_handshake_finish_batch_dev                       len is not 92: RG_PKT_INVALID
 *   rg_peer_cookie_consume_batch_dev                    len is not 64: RG_PKT_INVALID
 *   rg_recv_batch_dev_resident                          W < 16: no header read, no lookup, RG_PKT_INVALID from the open
 * A listed row carries key_idx 0: the chains only tell RG_KEY_SKIP from any other value.
 *
 * Per datagram the result of rg_demux_batch_dev equals this loop, bit for bit on every output byte:
 *   rank = {hs: 0, ck: 0, data: 0}; seen = {hs: 0, ck: 0, data: 0}
 *   for i in array order:
 *     d = desc[i]; cls[i] = 0; pos[i] = RG_KEY_SKIP
 *     d.key_idx == RG_KEY_SKIP                     -> RG_PKT_REJECTED, nothing read (an empty slot of the receive ring)
 *     d.offset % 16 != 0                           -> RG_PKT_UNALIGNED                   (lib.rs:613)
 *     d.len < 4, or d.offset + d.len > buf_len
 *     (in 64 bits, without wrapping)               -> RG_PKT_INVALID                     (lib.rs:620)
 *     t = the little-endian u32 at buf + d.offset
 *     t == 1: len == 148 ? list hs   : RG_PKT_INVALID   (handshake.rs:45, mut_from_bytes is exact-size)
 *     t == 2: len == 92  ? list hs   : RG_PKT_INVALID   (handshake.rs:149)
 *     t == 3: len == 64  ? list ck   : RG_PKT_INVALID   (handshake.rs:238)
 *     t == 4:              list data                    (the framing verdicts stay the receive's own)
 *     else                                         -> RG_PKT_INVALID                     (lib.rs:628)
 *     "list L": seen[L]++; k = rank[L]
 *        k < cap[L] -> rank[L]++; row k of L's arrays = d (key_idx written as 0) and addrs[i];
 *                      cls[i] = t; pos[i] = k; status[i] = RG_PKT_PENDING   (the verdict is the chain's)
 *        else       -> cls[i] = t; status[i] = RG_PKT_FULL                  (dropped, like a full socket buffer)
 *   counts[0..3) = rank, counts[3..6) = seen   (hs, ck, data)
 * computed as one ordered compaction over the n datagrams whose sum carries the three counts: the count walk reads
 * each datagram's type word once and leaves its class in cls, the rank walk reads cls and places the rows, and a pad
 * pass over the lists' capacities writes the inert tails behind counts[0..3).  RG_PKT_PENDING is the honest verdict
 * here: nothing has judged the message yet.
 *
 * rg_demux_verdict_batch_dev, one lane per datagram: for every i with status[i] == RG_PKT_PENDING,
 *   cls[i] == 1 or 2 and pos[i] < cap_hs   -> f = hs_filter_status[pos[i]]; f != RG_PKT_OK ? f
 *                                             : cls[i] == 1 ? init_status[pos[i]] : finish_status[pos[i]]
 *   cls[i] == 3 and pos[i] < cap_ck        -> cookie_status[pos[i]]
 *   cls[i] == 4 and pos[i] < cap_data      -> data_status[pos[i]]
 * Any of the five chain status pointers may be NULL: its datagrams stay RG_PKT_PENDING.  A pos out of range or a cls
 * outside 1-4 stays RG_PKT_PENDING and is never used as an index.  After this call status[n] is what a loop of
 * recv_message over the batch returns, in the caller's order.
 *
 * Unlike the reference: (a) a descriptor with key_idx == RG_KEY_SKIP is an empty slot and reads RG_PKT_REJECTED, where
 * the reference has no such thing as a datagram that did not arrive; (b) the lists have capacities, and a message past
 * its list's capacity reads RG_PKT_FULL and is dropped, where the reference handles one message at a time and can
 * never be full; (c) a type-4 datagram of any length is listed -- the reference's length and framing checks of a data
 * packet (lib.rs:635-650) run in rg_recv_batch_dev_resident, whose verdict the way back returns. */
typedef struct rg_demux_lists {      /* host struct, read at call time; every pointer is device memory */
    rg_pkt_desc *hs_desc;            /* [cap_hs] types 1 and 2 in array order */
    rg_src_addr *hs_addrs;           /* [cap_hs] */
    rg_pkt_desc *init_desc;          /* [cap_hs] row k: hs_desc[k] if type 1, else inert */
    rg_pkt_desc *resp_desc;          /* [cap_hs] row k: hs_desc[k] if type 2, else inert */
    rg_pkt_desc *ck_desc;            /* [cap_ck] type 3 */
    rg_pkt_desc *data_desc;          /* [cap_data] type 4 */
    rg_src_addr *data_addrs;         /* [cap_data] */
    uint32_t cap_hs, cap_ck, cap_data;
} rg_demux_lists;

size_t rg_demux_workspace_size(size_t n);
int rg_demux_batch_dev(rg_ctx *ctx, const rg_pkt_desc *desc /* [n] */, const rg_src_addr *addrs /* [n] */, size_t n,
                       const uint8_t *buf, size_t buf_len, const rg_demux_lists *lists /* host */,
                       uint8_t *status /* [n] */, uint8_t *cls /* [n] */, uint32_t *pos /* [n] */,
                       uint32_t *counts /* [6] */, void *workspace, size_t workspace_len, void *stream);
int rg_demux_verdict_batch_dev(rg_ctx *ctx, const uint8_t *cls /* [n] */, const uint32_t *pos /* [n] */, size_t n,
                               const uint8_t *hs_filter_status /* [cap_hs] or NULL */,
                               const uint8_t *init_status /* [cap_hs] or NULL */,
                               const uint8_t *finish_status /* [cap_hs] or NULL */, uint32_t cap_hs,
                               const uint8_t *cookie_status /* [cap_ck] or NULL */, uint32_t cap_ck,
                               const uint8_t *data_status /* [cap_data] or NULL */, uint32_t cap_data,
                               uint8_t *status /* [n] */, void *stream);

/* ------------------------------------------- several GPUs, one thread */
/* The reference's host is one thread owning one Sessions (RefCell, rustyguard-core/src/lib.rs:
 * 349-352; send_message / recv_message :542-583, :605-681).  A group lets that one thread drive
 * several GPUs: one context per entry of devices[] (a device may repeat: several contexts on one
 * GPU).  A batch given to a group is split into contiguous index ranges of about equal AEAD work
 * (payload bytes + one 64-byte key block per packet; rg_split_batch), one per context; every
 * context's H2D -> kernel -> D2H pipeline runs on its own streams, driven by a worker thread of the
 * library per context once some part spans more than two slices (rg_set_host_slice; smaller batches,
 * and contexts whose thread cannot be started, are stepped by the calling thread itself), and the call
 * returns when all are done.  The caller's
 * current device is left as it was.  Results are those of one context: the
 * packets are independent, counters are reserved before the split (rg_send_batch)
 * and the in-order anti-replay pass runs after the gather (rg_recv_batch_ex). */
typedef struct rg_group rg_group;
int rg_group_create(const int *devices, int n, rg_group **out);
void rg_group_destroy(rg_group *g);
int rg_group_size(const rg_group *g);
rg_ctx *rg_group_ctx(rg_group *g, int i); /* the i-th context (tuning knobs, device calls); NULL if out of range */
/* The split: bounds[0] = 0 <= bounds[1] <= ... <= bounds[parts] = n, part k = [bounds[k], bounds[k+1]),
 * cut where the running work (len, minus 32 when open, + 64 per packet) crosses k / parts of the total. */
int rg_split_batch(const rg_pkt_desc *desc, size_t n, int open, int parts, size_t *bounds);
/* rg_seal_batch_host / rg_open_batch_host over the group (same arguments and results). */
int rg_seal_batch_host_multi(rg_group *g, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                             const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *buf,
                             size_t buf_len, uint8_t *status);
int rg_open_batch_host_multi(rg_group *g, const uint8_t *keys, uint32_t nkeys, const rg_pkt_desc *desc, size_t n,
                             uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out);
/* Device-resident shards: shard i lives on context i's device (its own keys, descriptors, frames,
 * statuses and stream there); rg_seal_batch_dev / rg_open_batch_dev enqueued for every shard, from
 * this thread, without waiting (counters_out and receivers may be NULL as there).  Every shard's
 * arguments are checked before any shard is enqueued: RG_EINVAL names the bad shard and nothing ran.
 * A launch that fails after the checks (a device error) returns its code with rg_last_error naming
 * the shard k; shards 0..k-1 are enqueued, k and later are not. */
typedef struct rg_dev_shard {
    const uint8_t *keys;
    const uint32_t *receivers; /* seal only */
    uint32_t nkeys;
    const rg_pkt_desc *desc;
    const uint64_t *counters; /* seal only */
    size_t n;
    uint8_t *buf;
    size_t buf_len;
    uint8_t *status;
    uint64_t *counters_out; /* open only */
    void *stream;
} rg_dev_shard;
int rg_seal_batch_dev_multi(rg_group *g, const rg_dev_shard *shards);
int rg_open_batch_dev_multi(rg_group *g, const rg_dev_shard *shards);
/* A session table whose host-frame batches (rg_send_batch, rg_recv_batch[_ex]) run on the whole
 * group; the device-frame calls (rg_send_batch_dev, rg_recv_batch_dev) refuse such a table. */
int rg_sessions_create_group(rg_group *g, uint32_t capacity, rg_sessions **out);

/* ------------------------------------------------ synthetic workloads */
/* Device fill of payload bytes: inner bytes [0, inner_len[i]) of packet i
 * are le64(mix64(seed + (i << 16) + word)), bytes [inner_len, P) are zero.
 * desc/inner_len/buf are device pointers; desc[i].len = P. */
int rg_synth_fill_dev(rg_ctx *ctx, const rg_pkt_desc *desc, const uint32_t *inner_len, size_t n, uint8_t *buf,
                      size_t buf_len, uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RG_AEAD_H */
