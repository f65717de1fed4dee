// ibm_plan_check.cpp -- prints what fluca_amd/csrc/fl_ibm_plan.h plans for every rank of a rank grid, for tests/test_ibm_plan_host.py to judge.
// Plain C++: no HIP call; libflucahip.so is linked for fl_decomp_default / fl_decomp_neighbor_offset only.
//   usage: ibm_plan_check RX RY RZ PX PY PZ
//   C rank cx cy cz                                      the rank's coordinates
//   P rank code peer                                     for every offset code
//   M variant rank S|R code peer count offset sendtag recvtag   the messages in list order; offset in doubles from the start of the buffer
// variants: records (3 doubles per record, empty messages left out), keep (the same counts, empty messages kept), faces (the six-face exchange of
// ibm_neighbour_ranges: one record of 6 doubles from slot 0, received in slot 1 + code).
#include <cstdio>
#include <cstdlib>

#include "../../fluca_amd/csrc/fl_ibm_plan.h"

// the records rank `rank` sends under offset `code`: a fixed function that is zero for a quarter of the pairs
static int send_count(int rank, int code) { return (7 * rank + 3 * code + rank * code) % 4; }

static void print(const char *variant, int rank, const std::vector<fl::Msg> &msgs, double *sbuf, double *rbuf)
{
  for (const fl::Msg &m : msgs) {
    const bool send = m.send != nullptr;
    if (send == (m.recv != nullptr)) std::exit(3);  // a message is a send or a receive
    // Msg does not carry the offset code it was planned under: it is printed from the send tag, or for a receive from the receive tag.  What the
    // test asserts per rank about that tag of a receive is therefore empty; the pair test, the peer and the place in the buffer judge it
    std::printf("M %s %d %c %d %d %lld %lld %d %d\n", variant, rank, send ? 'S' : 'R', send ? m.sendtag : 26 - m.recvtag, m.peer, (long long)m.count, (long long)(send ? m.send - sbuf : m.recv - rbuf), m.sendtag,
                m.recvtag);
  }
}

int main(int argc, char **argv)
{
  if (argc != 7) return 2;
  int ranks[3], periodic[3];
  for (int d = 0; d < 3; ++d) ranks[d] = std::atoi(argv[1 + d]), periodic[d] = std::atoi(argv[4 + d]);
  const int     nranks = ranks[0] * ranks[1] * ranks[2];
  const int64_t n[3]   = {8 * ranks[0], 8 * ranks[1], 8 * ranks[2]};
  std::vector<fl_decomp> dec((size_t)nranks);
  std::vector<int>       peer(27 * (size_t)nranks);
  for (int r = 0; r < nranks; ++r) {
    if (fl_decomp_default(n, ranks, r, &dec[(size_t)r])) return 4;
    int lo[3], hi[3];
    fl::ibm_plan_peers(&dec[(size_t)r], periodic, lo, hi, &peer[27 * (size_t)r]);
    std::printf("C %d %d %d %d\n", r, dec[(size_t)r].coord[0], dec[(size_t)r].coord[1], dec[(size_t)r].coord[2]);
    for (int code = 0; code < 27; ++code) std::printf("P %d %d %d\n", r, code, peer[27 * (size_t)r + code]);
  }
  std::vector<double> sbuf(1 << 12), rbuf(1 << 12);
  for (int r = 0; r < nranks; ++r) {
    const int *pr = &peer[27 * (size_t)r];
    int        scnt[27], soff[27], rcnt[27], roff[27], so = 0, ro = 0;
    for (int code = 0; code < 27; ++code) {
      scnt[code] = pr[code] >= 0 ? send_count(r, code) : 0;
      rcnt[code] = pr[code] >= 0 ? send_count(pr[code], 26 - code) : 0;  // what the peer sends under the opposite offset
      soff[code] = so, so += scnt[code];
      roff[code] = ro, ro += rcnt[code];
    }
    std::vector<fl::Msg> msgs;
    fl::ibm_plan_msgs(pr, scnt, soff, rcnt, roff, 3, sbuf.data(), rbuf.data(), false, msgs);
    print("records", r, msgs, sbuf.data(), rbuf.data());
    fl::ibm_plan_msgs(pr, scnt, soff, rcnt, roff, 3, sbuf.data(), rbuf.data(), true, msgs);
    print("keep", r, msgs, sbuf.data(), rbuf.data());
    int one[27], zero[27], slot[27];
    for (int code = 0; code < 27; ++code) one[code] = 1, zero[code] = 0, slot[code] = 1 + code;
    fl::ibm_plan_msgs(pr, one, zero, one, slot, 6, sbuf.data(), rbuf.data(), true, msgs, fl::IBM_FACE_CODES);
    print("faces", r, msgs, sbuf.data(), rbuf.data());
  }
  return 0;
}
