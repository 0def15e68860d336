// What both pumps share around the integrity tags (csrc/kernels/integrity.h): the sabotage test hook and
// the text of a failed check.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string>

#include "kernels/launchers.h"

namespace eh {

// Test hook ERASUREHEAD_SABOTAGE=<what>:<rank>:<round> (what: msg | beta): the named put flips one
// payload byte after its checksum, so the receiver must report a torn message.  ("handshake:<rank>":
// that rank never answers the IPC handshake, parallel/transport.py.)  Read at every put, so a test can
// arm it for one Trainer of a process and disarm it before the next (bench.py first-contact ladder).
inline bool sabotage(const char* what, int rank, int round) {
  const char* e = std::getenv("ERASUREHEAD_SABOTAGE");
  if (e == nullptr || e[0] == '\0') return false;
  const std::string spec(e);
  return spec == std::string(what) + ":" + std::to_string(rank) + ":" + std::to_string(round);
}

inline std::string integrity_message(const IntegrityErr& e, bool beta) {
  char buf[512];
  if (beta)
    std::snprintf(buf, sizeof(buf),
                  "message integrity check failed: beta of round %d from rank %d: tag says round %d rank %u "
                  "checksum %016llx, payload checksum %016llx",
                  e.round, e.rank_want, static_cast<int>(e.round1_got) - 1, e.rank_got, e.sum_got, e.sum_calc);
  else
    std::snprintf(buf, sizeof(buf),
                  "message integrity check failed: round %d, rank %d's message in mailbox slot %d row %d: tag says "
                  "round %d rank %u checksum %016llx, payload checksum %016llx",
                  e.round, e.rank_want, e.where >> 16, e.where & 0xffff, static_cast<int>(e.round1_got) - 1, e.rank_got,
                  e.sum_got, e.sum_calc);
  return buf;
}

}  // namespace eh
