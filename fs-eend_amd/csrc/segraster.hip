// Reference segments -> the packed uint8 label rows that the collar DER reads (include/eend_hip.h at eend_segments_raster_u8): what
// metrics.read_rttm parsed goes to the device as a table of (recording, speaker, start frame, end frame) and becomes rows there,
// so no (T, C) matrix is built on the host.  Two launches on the caller's stream: seg_clear_kernel zeroes the rows (16-byte
// stores, bytes at the ragged end; a kernel and not a memset node, for the reason der_clear_kernel gives), then
// seg_raster_kernel, one workgroup per segment, stores a 1 per frame of the segment.  Overlapping segments of one speaker store
// the same value, so no order is needed and every run gives the same bytes.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT)
void seg_clear_kernel(unsigned char* __restrict__ rows, size_t nbytes) {
    const size_t at = ((size_t)blockIdx.x * NT + threadIdx.x) * 16;
    if (at + 16 <= nbytes) *(uint4*)(rows + at) = make_uint4(0u, 0u, 0u, 0u);
    else
        for (size_t k = at; k < nbytes; ++k) rows[k] = 0;
}

// A segment out of the table's domain (recording outside [0, B), speaker outside [0, C)) writes nothing; its frames are
// clipped to the recording's rows, and those to the nrows the buffer holds.
__global__ __launch_bounds__(NT)
void seg_raster_kernel(const int4* __restrict__ seg, const int* __restrict__ roff, int B, int C, unsigned char* __restrict__ rows,
                       long nrows) {
    const int4 s = seg[blockIdx.x];                               // recording, speaker, start, end
    if (s.x < 0 || s.x >= B || s.y < 0 || s.y >= C) return;
    const long r0 = roff[s.x], r1 = roff[s.x + 1];
    if (r0 < 0 || r1 > nrows || r1 < r0) return;
    const long len = r1 - r0;
    const long a = s.z > 0 ? s.z : 0, b = s.w < len ? s.w : len;
    unsigned char* const col = rows + (size_t)r0 * C + s.y;
    for (long f = a + threadIdx.x; f < b; f += NT) col[(size_t)f * C] = 1;
}

}  // namespace

int eend_launch_segments_raster(const int* seg, long nseg, const int* roff, int B, int C, unsigned char* rows, long nrows,
                                hipStream_t stream) {
    if (!roff || !rows || (nseg > 0 && !seg)) return EEND_EINVAL;
    if (B < 1 || B > 65535 || C < 1 || C > DER_CMAX || nseg < 0 || nseg > 0x7fffffffL || nrows < 1 || nrows > DER_MAX_FRAMES)
        return EEND_EINVAL;
    if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)seg & 15) != 0) return EEND_EINVAL;
    const size_t nbytes = (size_t)nrows * C;
    const size_t blocks = (nbytes + (size_t)NT * 16 - 1) / ((size_t)NT * 16);
    hipLaunchKernelGGL(seg_clear_kernel, dim3((unsigned)blocks), dim3(NT), 0, stream, rows, nbytes);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    if (nseg > 0) {
        hipLaunchKernelGGL(seg_raster_kernel, dim3((unsigned)nseg), dim3(NT), 0, stream, (const int4*)seg, roff, B, C, rows, nrows);
        if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    }
    return EEND_OK;
}
