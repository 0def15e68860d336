// Host entry points of the slab reduction (slab_reduce.hip).  dtype: the storage code of launchers.h (fp64 accumulators for 0 and 3, else fp32); slab,
// part (launchers.h slab_part_bytes) and G [nslots][ld] hold that type; stb [nslots + 1]: each message's slab rows.
#pragma once

#include "launchers.h"

namespace eh {

// The form set_slab_reduce_mode chose.  put (optional): the worker's message put + signal rides the final
// reduction kernel (put_protocol.h); put->gate must be `gate`.
hipError_t slab_reduce_launch(int dtype, const void* slab, const int* stb, void* part, void* G, int nslots, int ld,
                              hipStream_t st, const PutDesc* put = nullptr, const int* gate = nullptr);
// Stage 1, then stage 2 fused with a device-driven local round's combine + update (slab_final_update).
hipError_t slab_reduce_update_launch(int dtype, const void* slab, const int* stb, void* part, void* G, int nslots,
                                     int ld, hipStream_t st, const LocalUpdate& up);

}  // namespace eh
