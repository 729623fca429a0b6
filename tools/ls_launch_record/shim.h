// Force-included (-include) in front of csrc/rls_localsearch.hip (or rls_mcpg.hip) by record.py: every hipLaunchKernelGGL of the file
// becomes a call of the recorder in main.cpp -- kernel pointer, grid, block, dynamic LDS and every kernel argument (structs by their
// size) -- and nothing is launched.
#ifndef RLS_LS_LAUNCH_RECORD_SHIM_H
#define RLS_LS_LAUNCH_RECORD_SHIM_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>

namespace ls_rec {
void begin(const void* kern, dim3 grid, dim3 block, size_t lds);
void arg_ptr(const void* p);
void arg_int(long long v);
void end();
template <class T>
inline void arg(T v) {
    if constexpr (std::is_pointer_v<T>) arg_ptr((const void*)v);
    else if constexpr (std::is_arithmetic_v<T> || std::is_enum_v<T>) arg_int((long long)v);
    else arg_int(-(long long)sizeof(T));
}
template <class... A>
inline void record(const void* kern, dim3 grid, dim3 block, size_t lds, A... a) {
    begin(kern, grid, block, lds);
    (arg(a), ...);
    end();
}
}  // namespace ls_rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) \
    ::ls_rec::record((const void*)(kern), dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__)
#endif
