// boundary.h -- what an extern "C" entry point needs besides its own module: the capture query and the two pointer
// predicates every argument check is written in (internal).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/gsplat_mi355.h"

// ---- stream capture (hipGraph; capi.hip has the history).  An entry point enqueues kernel nodes only on a capturing
// stream and answers GS_E_CAPTURE -- before enqueuing anything -- to a call that would need more.
bool stream_is_capturing(void* stream);
bool profiling_on();  // the stage timer (event nodes)
// capture-safe entry points: refuse debug mode (it synchronises) and the stage timer under capture
#define GS_CAPTURE_OK_IF(stream, cond)                                           \
    do {                                                                         \
        if (stream_is_capturing(stream) && (!(cond) || profiling_on())) return GS_E_CAPTURE; \
    } while (0)
#define GS_NO_CAPTURE(stream) GS_CAPTURE_OK_IF(stream, false)

// ---- pointers: `bytes` is the widest access the kernels make through p (16: float4 / dwordx4, 4: scalar floats)
// an optional pointer: null, or aligned to `bytes`
static inline bool aligned(const void* p, size_t bytes) { return (uintptr_t)p % bytes == 0; }
// a required pointer: non-null and aligned to `bytes`
static inline bool required(const void* p, size_t bytes) { return p != nullptr && aligned(p, bytes); }
