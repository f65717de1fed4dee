// fl_ibm_plan.h -- the host arithmetic of the owner-rank markers' messages (fl_ibm_owner.hip): which of the 27 neighbour offsets have a rank behind
// them, and THE list of one exchange.  Needs nothing from HIP, so that a plain C++ program can check it for every rank of a rank grid
// (tests/test_ibm_plan_host.py).
// Neighbour offsets o in {-1,0,1}^3 are numbered code = (oz+1)*9 + (oy+1)*3 + (ox+1); 13 is the block itself, 26 - code the opposite offset.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/fluca_hip.h"
#include "fl_msg.h"

#pragma GCC visibility push(hidden)  // internal to the library that includes it

namespace fl {

constexpr unsigned IBM_ALL_CODES  = (1u << 27) - 1u;
constexpr unsigned IBM_FACE_CODES = 1u << 4 | 1u << 10 | 1u << 12 | 1u << 14 | 1u << 16 | 1u << 22;  // the offsets with one non-zero entry

// peer_lo / peer_hi[d]: a rank sits behind the low / high end of the block along axis d (not a wall, not an axis one rank holds alone);
// peer[code]: the rank behind the offset, -1 where there is none (13, the block itself, included)
inline void ibm_plan_peers(const fl_decomp *dec, const int periodic[3], int peer_lo[3], int peer_hi[3], int peer[27])
{
  for (int d = 0; d < 3; ++d) {
    const bool sp = dec->ranks[d] > 1;
    peer_lo[d]    = sp && (dec->coord[d] > 0 || periodic[d]);
    peer_hi[d]    = sp && (dec->coord[d] < dec->ranks[d] - 1 || periodic[d]);
  }
  for (int code = 0; code < 27; ++code) {
    const int o[3] = {code % 3 - 1, (code / 3) % 3 - 1, code / 9 - 1};
    bool      ok   = code != 13;
    for (int d = 0; d < 3; ++d) ok = ok && (o[d] == 0 || (o[d] < 0 ? peer_lo[d] : peer_hi[d]));
    peer[code] = ok ? fl_decomp_neighbor_offset(dec, periodic, o) : -1;
  }
}

// The messages of one exchange with the neighbours: under offset `code` this rank sends scnt[code] records of `per` doubles that start at record
// soff[code] of sbuf, and receives rcnt[code] records at record roff[code] of rbuf.  Sends in ascending offset code; receives in the order the peer
// sends, which is DESCENDING code here (the peer numbers the same pair of blocks 26 - code): RCCL matches the messages between two ranks by order,
// and two offsets may lead to the same rank (two ranks on a periodic axis) -- fl_halo_plan's rule.  The tags say the same for a transport that
// carries them.  An empty message is left out unless keep_empty (both sides must know every count to leave one out); codes: the offsets that take part.
inline void ibm_plan_msgs(const int peer[27], const int scnt[27], const int soff[27], const int rcnt[27], const int roff[27], int per, double *sbuf, double *rbuf, bool keep_empty,
                          std::vector<Msg> &msgs, unsigned codes = IBM_ALL_CODES)
{
  msgs.clear();
  for (int code = 0; code < 27; ++code)
    if (peer[code] >= 0 && (codes >> code & 1u) && (keep_empty || scnt[code] > 0)) msgs.push_back({peer[code], sbuf + (int64_t)per * soff[code], nullptr, (int64_t)per * scnt[code], code, 26 - code});
  for (int code = 26; code >= 0; --code)
    if (peer[code] >= 0 && (codes >> code & 1u) && (keep_empty || rcnt[code] > 0)) msgs.push_back({peer[code], nullptr, rbuf + (int64_t)per * roff[code], (int64_t)per * rcnt[code], code, 26 - code});
}

}  // namespace fl

#pragma GCC visibility pop
