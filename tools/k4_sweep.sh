# Tuning aid: split-K kernels against the uniform-wave kernels (split-K switched off) per layer and batch size.
#   K4_BATCHES="2 4 8" PP_SEP_K4=8 PP_DECONV_K4=8 bash tools/k4_sweep.sh
for B in ${K4_BATCHES:-2 4 8 16}; do
  echo "== B=$B split-K where selected"
  python tools/layer_bench.py --batch $B
  echo "== B=$B uniform-wave"
  PP_SEP_K4=0 PP_DECONV_K4=0 python tools/layer_bench.py --batch $B
done
