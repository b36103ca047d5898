// The shared-key-prefix instantiations of attn_kernel (SH = true) and launch_attention_shared: the kernel template comes from
// attention.hip, compiled here with its own launchers switched off, so that the existing instantiations build exactly as before.
#define LR_ATT_SHARED_TU 1
#include "attention.hip"
