// fast_vn_dec.hip -- explicit instantiation of one group of specialised-kernel launchers (see kernels_fast.hpp)
#include "kernels_fast.hpp"
namespace lutldpc {
template bool launch_vn_fast<TT_DEC, 1> LUTLDPC_CLASS_SIG;
template bool launch_vn_fast<TT_DEC, 2> LUTLDPC_CLASS_SIG;
template hipError_t preload_vn_fast<TT_DEC, 2>();
}
