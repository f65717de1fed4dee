// fl_msg.h -- one message of an exchange (Comm::exchange, fl_comm.hip).  Needs nothing from HIP: host-only headers that plan messages include it.
#pragma once
#include <cstdint>

namespace fl {

struct Msg {
  int     peer;
  double *send, *recv;  // device
  int64_t count;
  int     sendtag, recvtag;
};

}  // namespace fl
