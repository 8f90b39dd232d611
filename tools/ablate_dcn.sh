#!/bin/bash
# builds tools/_libctdet_dcnabl{1,2}.so: the library with conv_f32.hip compiled under -DCTDET_DCN_ABLATE=N (measurement only;
# results of these builds are wrong by design: conv_f32.hip says what each bit drops)
set -e
cd "$(dirname "$0")/../detectron2-centernet_amd/csrc"
for n in ${@:-1 2}; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-function -Wno-inline-asm -DCTDET_DCN_ABLATE=$n -c conv_f32.hip -o /tmp/conv_f32_abl$n.o
  objs=$(ls ../lib/obj/*.o | grep -v conv_f32.o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/_libctdet_dcnabl$n.so $objs /tmp/conv_f32_abl$n.o -ldl
done
