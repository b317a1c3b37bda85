// The camera renderer a second time, with the opt-in effects (mmx_set_render_effects):
// mmx_render_lit_kernel (cast shadows of the directional light, the bins blended at alpha 0.4),
// mmx_shadow_kernel (the per-env height map the shadow test reads) and their launcher
// mmx_launch_render_lit, which mmx_launch_render calls when its `flags` argument names an effect.
// Same sources, same rasteriser, same depth keys: segment ids and every pixel no effect touches are
// bit-identical to the flat kernel's, whose code object this leaves untouched.
#define MMR_LIT 1
#include "mmx_render.hip"
