// fast_cn.hip -- explicit instantiation of one group of specialised-kernel launchers (see kernels_fast.hpp)
#include "kernels_fast.hpp"
namespace lutldpc {
template bool launch_cn_fast<1> LUTLDPC_CLASS_SIG;
template bool launch_cn_fast<2> LUTLDPC_CLASS_SIG;
template hipError_t preload_cn_fast<2>();
}
