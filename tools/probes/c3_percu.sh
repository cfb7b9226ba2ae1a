# needs the profiling build of the library: make EXTRA=-DQT_PROFILING_VARIANTS OUT=../lib/libqt_hip_prof.so, then QT_HIP_LIB=<that library>
for pc in 2 1; do echo "PER_CU $pc"; QT_C3_PER_CU=$pc bash tools/probes/c4_kt.sh 2>&1 | grep -i "code_conv3x3"; done
