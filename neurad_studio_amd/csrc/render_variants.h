// The fused render kernel's variants (render.hip: nrhip::render_kernel): how a variant is named, which mixes are legal, and
// THE list of the ones that are instantiated.  Everything that has to know "which kernels exist" is derived from the list:
// the launch switch, validate_field and its error text (render.hip); the host-side gate in fields/neurad_field.py is
// pinned to it by tests/test_fused_shapes_gate.py, which parses this file.
#pragma once

namespace nrhip {

// what the kernel writes
enum class Out {
  PerSample,  // feature / sdf / alpha of every sample (field forward; training forward when activations are saved)
  Composite,  // C1 + C2 fused: features / depth / accumulation per ray
};
// where a sample's encoding comes from
enum class Src {
  Static,     // the static scene's hash table
  EvalTable,  // the same table in the eval layout (eval_layout.hip: coarse levels read from their shadow copies)
  Actors,     // per-sample table select: a sample inside an actor's box reads that actor's grid
  Overrides,  // samples inside an actor box take encoding row and view direction from the caller (training)
};
// how the four per-tile matrix products are formed
enum class Prod {
  F32,        // v_mfma_f32_16x16x4_f32
  Bf16Split,  // 3-way split bf16 (mfma_layer_split)
  F16Pairs,   // fp16 pairs (mfma_layer_pairs)
};

// how a ray's samples are addressed
enum class Lay {
  Dense,   // [R, S] with a row stride: every ray has S samples
  Packed,  // [M] + segments [R + 1]: ray r owns the samples [segments[r], segments[r + 1]) (the occupancy march's output)
  PackedRows,  // the same addressing for the per-sample kernel: every output and saved row at the packed sample index
  PackedActors,  // Packed for a scene with dynamic actors: the composited kernel with the per-sample table select
  PackedRowsOvr,  // PackedRows with row overrides: the packed training forward of a scene with dynamic actors
};

// The legal mixes, asserted by the kernel for every instantiation.
constexpr bool render_variant_ok(int L, int F, Out out, Src src, Prod prod, Lay lay = Lay::Dense) {
  // packed samples: the composited static-scene kernel, fp32 or pair products.  The packed kernels have no rows of their
  // own below: every row this rule admits is instantiated in both layouts (render.hip: packed_lay, launch_row)
  if (lay == Lay::Packed && !(out == Out::Composite && src == Src::Static && prod != Prod::Bf16Split)) return false;
  // ... and the per-sample static-scene kernel with fp32 products (the packed training forward), derived the same way
  if (lay == Lay::PackedRows && !(out == Out::PerSample && src == Src::Static && prod == Prod::F32)) return false;
  // ... and the composited actor kernel, fp32 products: every `Composite, Actors, F32` row, derived the same way
  if (lay == Lay::PackedActors && !(out == Out::Composite && src == Src::Actors && prod == Prod::F32)) return false;
  // ... and the per-sample kernel with row overrides, fp32 products: every `PerSample, Overrides, F32` row, derived the
  // same way
  if (lay == Lay::PackedRowsOvr && !(out == Out::PerSample && src == Src::Overrides && prod == Prod::F32)) return false;
  // actors (static and actor tables share one storage type) and the eval-table layout: the composited eval kernel
  if ((src == Src::Actors || src == Src::EvalTable) && out != Out::Composite) return false;
  // row overrides: the per-sample training forward
  if (src == Src::Overrides && out != Out::PerSample) return false;
  // split / pair products: static-scene kernels (the relayout and the split / pair products do not combine) ...
  if (prod != Prod::F32 && src != Src::Static) return false;
  // ... and, like the eval-table layout, the full frame only
  if ((prod != Prod::F32 || src == Src::EvalTable) && L * F != 32) return false;
  // the 3-way bf16 split: the composited kernel.  (fp16 pairs: also the per-sample kernel -- the training forward: the tile
  // runs in units of kPairAct, every store of an activation undoes it)
  if (prod == Prod::Bf16Split && out != Out::Composite) return false;
  return true;
}

}  // namespace nrhip

// X(L, F, H, output, source, products): one line per instantiation; every line exists for fp32 and fp16 tables, and every
// `Composite, Static` line with `F32` or `F16Pairs` products for dense and packed samples, every `PerSample, Static, F32`
// line for dense samples and packed rows, every `Composite, Actors, F32` line for dense and packed samples, every
// `PerSample, Overrides, F32` line for dense samples and packed rows (render_variant_ok).
// L * F == 32 (L = 16, 8, 4) fills the kernel's encoding frame; the smaller grids live in the padded frame (EncFrame):
// BASELINE config[0]'s 1 x 4, NeuRAD tiny's 4 x 2, and the L * F == 16 grids 4 x 4 and 8 x 2 -- fp32 products only.
#define NRHIP_RENDER_VARIANTS(X)        \
  X(16, 2, 64, Composite, Static, F32)  \
  X(16, 2, 32, Composite, Static, F32)  \
  X(8, 4, 32, Composite, Static, F32)   \
  X(8, 4, 64, Composite, Static, F32)   \
  X(4, 8, 32, Composite, Static, F32)   \
  X(4, 8, 64, Composite, Static, F32)   \
  X(1, 4, 32, Composite, Static, F32)   \
  X(1, 4, 64, Composite, Static, F32)   \
  X(4, 2, 32, Composite, Static, F32)   \
  X(4, 2, 64, Composite, Static, F32)   \
  X(4, 4, 32, Composite, Static, F32)   \
  X(4, 4, 64, Composite, Static, F32)   \
  X(8, 2, 32, Composite, Static, F32)   \
  X(8, 2, 64, Composite, Static, F32)   \
  X(16, 2, 64, PerSample, Static, F32)  \
  X(16, 2, 32, PerSample, Static, F32)  \
  X(8, 4, 32, PerSample, Static, F32)   \
  X(8, 4, 64, PerSample, Static, F32)   \
  X(4, 8, 32, PerSample, Static, F32)   \
  X(4, 8, 64, PerSample, Static, F32)   \
  X(1, 4, 32, PerSample, Static, F32)   \
  X(1, 4, 64, PerSample, Static, F32)   \
  X(4, 2, 32, PerSample, Static, F32)   \
  X(4, 2, 64, PerSample, Static, F32)   \
  X(4, 4, 32, PerSample, Static, F32)   \
  X(4, 4, 64, PerSample, Static, F32)   \
  X(8, 2, 32, PerSample, Static, F32)   \
  X(8, 2, 64, PerSample, Static, F32)   \
  /* fp16 pairs: the composited kernel (64-wide, and NeuRAD's own width) ... */ \
  X(16, 2, 64, Composite, Static, F16Pairs) \
  X(8, 4, 64, Composite, Static, F16Pairs)  \
  X(4, 8, 64, Composite, Static, F16Pairs)  \
  X(16, 2, 32, Composite, Static, F16Pairs) \
  X(8, 4, 32, Composite, Static, F16Pairs)  \
  X(4, 8, 32, Composite, Static, F16Pairs)  \
  /* ... and the per-sample kernel (opt-in) */ \
  X(8, 4, 32, PerSample, Static, F16Pairs)  \
  X(16, 2, 64, PerSample, Static, F16Pairs) \
  X(8, 4, 64, PerSample, Static, F16Pairs)  \
  X(16, 2, 32, PerSample, Static, F16Pairs) \
  /* 3-way bf16 split (opt-in): 64-wide MLPs */ \
  X(16, 2, 64, Composite, Static, Bf16Split) \
  X(8, 4, 64, Composite, Static, Bf16Split)  \
  X(4, 8, 64, Composite, Static, Bf16Split)  \
  /* eval-table layout */ \
  X(16, 2, 64, Composite, EvalTable, F32) \
  X(8, 4, 32, Composite, EvalTable, F32)  \
  X(8, 4, 64, Composite, EvalTable, F32)  \
  /* dynamic actors: the static shapes NeuRAD uses with actors (4 x 2: NeuRAD tiny) -- eval ... */ \
  X(8, 4, 32, Composite, Actors, F32)  \
  X(8, 4, 64, Composite, Actors, F32)  \
  X(16, 2, 64, Composite, Actors, F32) \
  X(4, 2, 32, Composite, Actors, F32)  \
  X(4, 2, 64, Composite, Actors, F32)  \
  /* ... and the training forward with row overrides */ \
  X(8, 4, 32, PerSample, Overrides, F32)  \
  X(8, 4, 64, PerSample, Overrides, F32)  \
  X(16, 2, 64, PerSample, Overrides, F32) \
  X(4, 2, 32, PerSample, Overrides, F32)  \
  X(4, 2, 64, PerSample, Overrides, F32)
