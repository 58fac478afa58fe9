// peer_args.h -- the sizes of the peer mailboxes and a reduction's view of them (peer_kernels.h has the protocol and the kernels).
#pragma once

#include <stdint.h>

namespace ciao {

constexpr int PEER_MAX = 8;
constexpr int64_t PEER_HDR = 1024;        // flags: [2 parities][8 ranks] x 64 bytes
constexpr unsigned long long PEER_TICKS_PER_S = 100000000ull;   // s_memrealtime: the 100 MHz constant clock
constexpr int64_t PEER_WAIT_S_DEFAULT = 30;   // a reduction between ranks that run the same kernels: far more than any skew
                                              // (option peer_timeout_s; the chain owner's broadcast waits for a whole chain: broadcast_from_owner, api_solvers.hip)

struct PeerDev {
    int world, rank;                   // world == 0: no peers (single device, or the hook path)
    unsigned int seq;                  // this reduction's sequence number (>= 1; the same on every rank)
    int64_t slot_bytes;
    unsigned char *mail[PEER_MAX];     // mail[r] = rank r's mailbox (mail[rank] = own; the others IPC-mapped)
    unsigned int *counter;             // device-scope "workgroups done" counter of the sending kernel (this rank's own memory)
    int *errflag;
    unsigned long long wait_ticks;     // how long peer_wait() waits for a rank before it gives up (realtime ticks)
};

}  // namespace ciao
