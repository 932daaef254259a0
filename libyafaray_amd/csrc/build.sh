#!/bin/bash
# Builds libyafaray_gpu.so (HIP kernels + narrow ABI + Interface-shaped C API) for gfx950, in-tree.
# Objects are rebuilt only when their source, any header here or in include/, this script or the flags changed
# (YAFGPU_FORCE=1 rebuilds everything).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${YAFGPU_OUT:-$HERE/../libyafaray_gpu.so}"
OBJ="${YAFGPU_OBJ:-$HERE/obj}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# -ffp-contract=off and IEEE divide/sqrt: the shading arithmetic must round like the reference's
# expressions (discrete hit / lobe / shadow decisions decide image parity)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function"
EXTRA="${YAFGPU_EXTRA_FLAGS:-}"
mkdir -p "$OBJ"
HEADERS=("$HERE"/*.h "$HERE"/../../include/*.h "$HERE/yafaray_ies.cpp" "$HERE/build.sh")
STAMP="$OBJ/.flags"
if [ ! -f "$STAMP" ] || [ "$(cat "$STAMP")" != "$FLAGS $EXTRA" ] || [ "${YAFGPU_FORCE:-0}" = "1" ]; then rm -f "$OBJ"/*.o; echo "$FLAGS $EXTRA" > "$STAMP"; fi

stale() {   # stale <object> <source>: true when the object must be rebuilt
  local o="$1" s="$2" h
  [ -f "$o" ] || return 0
  [ "$s" -nt "$o" ] && return 0
  for h in "${HEADERS[@]}"; do [ "$h" -nt "$o" ] && return 0; done
  return 1
}
PIDS=()
cc() {      # cc <object name> <source> [defines...]: compile in the background when stale
  local o="$OBJ/$1.o" s="$HERE/$2"; shift 2
  if stale "$o" "$s"; then "$HIPCC" $FLAGS "$@" -c "$s" -o "$o" $EXTRA & PIDS+=($!); fi
}
# the device unit and the scene-specialised shading kernels (yafgpu_shade_variant.hip) compile side by side; every variant is built for
# area and point lights (YAFGPU_LIGHT_MASK=0x3u): scenes with directional, sun or sphere lights take the device unit's general kernel;
# none but the blend material's unit has ambient occlusion (YAFGPU_FEAT_AO=0): a render with do_AO takes the general kernel too
cc yafgpu_device yafgpu_device.hip
#   diffuse: shinydiffusemat + light_mat, no recursiveRaytrace (BASELINE configs C2, C3)
cc shade_diffuse yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=diffuse -DYAFGPU_MAT_MASK=0x5u -DYAFGPU_LIGHT_MASK=0x3u -DYAFGPU_FEAT_RECURSE=0 -DYAFGPU_FEAT_TEXTURE=0 -DYAFGPU_FEAT_ANISO=0 -DYAFGPU_FEAT_AO=0 -DYAFGPU_FEAT_MULTI=0
#   glossy: + glossy (as_diffuse), no recursiveRaytrace (C4)
cc shade_glossy yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=glossy -DYAFGPU_MAT_MASK=0x7u -DYAFGPU_LIGHT_MASK=0x3u -DYAFGPU_FEAT_RECURSE=0 -DYAFGPU_FEAT_TEXTURE=0 -DYAFGPU_FEAT_ANISO=0 -DYAFGPU_FEAT_AO=0 -DYAFGPU_FEAT_MULTI=0
#   ... the two with a second MIS pair per park (YAFGPU_FEAT_MULTI): scenes with several lights or several samples per light (C4)
cc shade_diffuse_mp yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=diffuse_mp -DYAFGPU_MAT_MASK=0x5u -DYAFGPU_LIGHT_MASK=0x3u -DYAFGPU_FEAT_RECURSE=0 -DYAFGPU_FEAT_TEXTURE=0 -DYAFGPU_FEAT_ANISO=0 -DYAFGPU_FEAT_AO=0 -DYAFGPU_FEAT_MULTI=1
cc shade_glossy_mp yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=glossy_mp -DYAFGPU_MAT_MASK=0x7u -DYAFGPU_LIGHT_MASK=0x3u -DYAFGPU_FEAT_RECURSE=0 -DYAFGPU_FEAT_TEXTURE=0 -DYAFGPU_FEAT_ANISO=0 -DYAFGPU_FEAT_AO=0 -DYAFGPU_FEAT_MULTI=1
#   ... and the two as the program of a serial-state replay's record pass (no light estimate, the vertex of a resume in registers)
cc shade_diffuse_rec yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=diffuse_rec -DYAFGPU_MAT_MASK=0x5u -DYAFGPU_LIGHT_MASK=0x3u -DYAFGPU_FEAT_RECURSE=0 -DYAFGPU_FEAT_TEXTURE=0 -DYAFGPU_FEAT_ANISO=0 -DYAFGPU_FEAT_AO=0 -DYAFGPU_FEAT_LIGHTS=0
cc shade_glossy_rec yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=glossy_rec -DYAFGPU_MAT_MASK=0x7u -DYAFGPU_LIGHT_MASK=0x3u -DYAFGPU_FEAT_RECURSE=0 -DYAFGPU_FEAT_TEXTURE=0 -DYAFGPU_FEAT_ANISO=0 -DYAFGPU_FEAT_AO=0 -DYAFGPU_FEAT_LIGHTS=0
#   full: every material type and recursiveRaytrace, no shader nodes / textures (the main unit's kernel has those too)
cc shade_full yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=full -DYAFGPU_MAT_MASK=0x3fu -DYAFGPU_LIGHT_MASK=0x3u -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=0 -DYAFGPU_FEAT_ANISO=0 -DYAFGPU_FEAT_AO=0 -DYAFGPU_FEAT_MULTI=0
#   blend: the device unit's general kernel (every material type, light type and feature: nothing else is switched off) with BlendMaterial's
#   code, bit 8 of the material mask; a scene takes it when some triangle uses a blend_mat, for the record pass of a serial-state replay too
cc shade_blend yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=blend -DYAFGPU_MAT_MASK=0x17fu -DYAFGPU_LIGHT_MASK=0x3fu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
#   meshlight, blend_meshlight: the general kernel and the blend's with MeshLight's code, bit 7 of the light mask (YAFGPU_LIGHT_MESH); a scene takes
#   one of them when it has a mesh light, so that every other scene's kernels stay what they were
cc shade_meshlight yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=meshlight -DYAFGPU_MAT_MASK=0x7fu -DYAFGPU_LIGHT_MASK=0xbfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
cc shade_blend_meshlight yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=blend_meshlight -DYAFGPU_MAT_MASK=0x17fu -DYAFGPU_LIGHT_MASK=0xbfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
#   portal, blend_portal: the same two with BackgroundPortalLight's code as well, bit 8 of the light mask (YAFGPU_LIGHT_PORTAL); a scene takes one of
#   them when it has a portal light, with or without a mesh light beside it
cc shade_portal yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=portal -DYAFGPU_MAT_MASK=0x7fu -DYAFGPU_LIGHT_MASK=0x1bfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
cc shade_blend_portal yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=blend_portal -DYAFGPU_MAT_MASK=0x17fu -DYAFGPU_LIGHT_MASK=0x1bfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
#   ies, blend_ies: the same two with IesLight's two types as well, bits 9 and 10 of the light mask (YAFGPU_LIGHT_IES, YAFGPU_LIGHT_IES_SOFT): every
#   light type's code; a scene takes one of them when it has an IES light of either kind, whatever other lights it has
cc shade_ies yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=ies -DYAFGPU_MAT_MASK=0x7fu -DYAFGPU_LIGHT_MASK=0x7bfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
cc shade_blend_ies yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=blend_ies -DYAFGPU_MAT_MASK=0x17fu -DYAFGPU_LIGHT_MASK=0x7bfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
#   spot, blend_spot: the same two with SpotLight's two types as well, bits 11 and 12 of the light mask (YAFGPU_LIGHT_SPOT, YAFGPU_LIGHT_SPOT_SOFT): every
#   light type's code; a scene takes one of them when it has a spot light of either kind, whatever other lights it has (an IES light included)
cc shade_spot yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=spot -DYAFGPU_MAT_MASK=0x7fu -DYAFGPU_LIGHT_MASK=0x1fbfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
cc shade_blend_spot yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=blend_spot -DYAFGPU_MAT_MASK=0x17fu -DYAFGPU_LIGHT_MASK=0x1fbfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1
#   sky, blend_sky: the same two with the evaluation of the gradient and sunsky backgrounds as well (YAFGPU_FEAT_SKY, yafgpu_texture.h: bg_eval); a scene
#   takes one of them when its background is one of the two, whatever lights it has, so that every other scene's kernels stay what they were
cc shade_sky yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=sky -DYAFGPU_MAT_MASK=0x7fu -DYAFGPU_LIGHT_MASK=0x1fbfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1 -DYAFGPU_FEAT_SKY=1
cc shade_blend_sky yafgpu_shade_variant.hip -DYAFGPU_VARIANT_NAME=blend_sky -DYAFGPU_MAT_MASK=0x17fu -DYAFGPU_LIGHT_MASK=0x1fbfu -DYAFGPU_FEAT_RECURSE=1 -DYAFGPU_FEAT_TEXTURE=1 -DYAFGPU_FEAT_ANISO=1 -DYAFGPU_FEAT_AO=1 -DYAFGPU_FEAT_MULTI=1 -DYAFGPU_FEAT_SKY=1
# scene set-up for instanced geometry: the rows of the flattened scene, made on the device (same flags: its arithmetic must round like the host loop's)
cc yafgpu_assemble yafgpu_assemble.hip
# the output stage: film -> packed pixels of an image file (same flags: its arithmetic must round like the host's deliver_to)
cc yafgpu_output yafgpu_output.hip
cc kdtree_build kdtree_build.cpp
cc kdtree_build_device kdtree_build_device.hip
OBJS="$OBJ/yafgpu_device.o $OBJ/shade_diffuse.o $OBJ/shade_glossy.o $OBJ/shade_diffuse_mp.o $OBJ/shade_glossy_mp.o $OBJ/shade_diffuse_rec.o $OBJ/shade_glossy_rec.o $OBJ/shade_full.o $OBJ/shade_blend.o $OBJ/shade_meshlight.o $OBJ/shade_blend_meshlight.o $OBJ/shade_portal.o $OBJ/shade_blend_portal.o $OBJ/shade_ies.o $OBJ/shade_blend_ies.o $OBJ/shade_spot.o $OBJ/shade_blend_spot.o $OBJ/shade_sky.o $OBJ/shade_blend_sky.o $OBJ/yafgpu_assemble.o $OBJ/yafgpu_output.o $OBJ/kdtree_build.o $OBJ/kdtree_build_device.o"
# (yafaray_ies.cpp, the IES file parser, is part of yafaray_c_api's unit: it is included there)
for f in yafaray_c_api yafaray_xml yafaray_image yafaray_reduce; do
  if [ -f "$HERE/$f.cpp" ]; then cc "$f" "$f.cpp"; OBJS="$OBJS $OBJ/$f.o"; fi
done
for p in "${PIDS[@]:-}"; do [ -n "$p" ] && wait "$p"; done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT" $OBJS -lpthread -lz ${YAFGPU_LINK_LIBS:-}
echo "built $OUT"
