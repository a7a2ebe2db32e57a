# The one build recipe: every native library of the package, the CPU oracle and the test libraries,
# in-tree.  __graft_entry__.build() runs the `all` target.
HIPCC ?= /opt/rocm/bin/hipcc
HIPFLAGS ?= --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -Wall
ENGINE := sctools_amd/libsctools_gpu.so
SRC := sctools_amd/csrc/sct_engine.hip
HDRS := $(filter-out sctools_amd/csrc/gbam_%.h,$(wildcard sctools_amd/csrc/*.h)) include/sctools_gpu.h

BAMDEC := sctools_amd/libsct_bam.so
CSVFMT := sctools_amd/libsct_csv.so
GBAM := sctools_amd/libsct_gbam.so
BARCODE := sctools_amd/libsct_barcode.so
FASTQ := sctools_amd/libsct_fastq.so

SI4 := tests/native/libsct_engine_si4.so

all: $(ENGINE) $(BAMDEC) $(CSVFMT) $(GBAM) $(BARCODE) $(FASTQ) oracle/liboracle.so tests/native/libfxcheck.so tests/native/libstdhash.so tests/native/libtsround.so tests/native/libfqcrc.so $(SI4)

$(ENGINE): $(SRC) $(HDRS)
	$(HIPCC) $(HIPFLAGS) -o $@ $(SRC) -L/opt/rocm/lib -lrccl

# test infrastructure: the engine with 1024-item radix tiles (tests/test_gpu_tagsort.py)
$(SI4): $(SRC) $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DSCT_SORT_ITEMS=4 -o $@ $(SRC) -L/opt/rocm/lib -lrccl

$(BAMDEC): sctools_amd/csrc/bamdec.cpp sctools_amd/csrc/bamsplit.cpp sctools_amd/csrc/bamtag.cpp sctools_amd/csrc/bamshards.cpp sctools_amd/csrc/bamwrite.h sctools_amd/csrc/bgzf.h include/sct_bam.h
	g++ -O3 -std=c++17 -fopenmp -fPIC -shared -Wall -o $@ sctools_amd/csrc/bamdec.cpp sctools_amd/csrc/bamsplit.cpp sctools_amd/csrc/bamtag.cpp sctools_amd/csrc/bamshards.cpp -lz

$(GBAM): sctools_amd/csrc/gbam.hip $(wildcard sctools_amd/csrc/gbam_*.h) sctools_amd/csrc/inflate.h sctools_amd/csrc/bgzf.h include/sct_gbam.h include/sct_bam.h
	$(HIPCC) $(HIPFLAGS) -o $@ sctools_amd/csrc/gbam.hip -lz

$(BARCODE): sctools_amd/csrc/barcode.hip sctools_amd/csrc/liberr.h include/sct_barcode.h
	$(HIPCC) $(HIPFLAGS) -o $@ sctools_amd/csrc/barcode.hip

$(FASTQ): sctools_amd/csrc/fastq.hip sctools_amd/csrc/fqmetrics.h sctools_amd/csrc/fqprocess.h sctools_amd/csrc/fqinflate.h sctools_amd/csrc/inflate.h sctools_amd/csrc/liberr.h include/sct_fastq.h include/sct_fastq_metrics.h include/sct_fastq_process.h include/sct_fastq_inflate.h
	$(HIPCC) $(HIPFLAGS) -o $@ sctools_amd/csrc/fastq.hip

$(CSVFMT): sctools_amd/csrc/csvfmt.cpp include/sct_csv.h
	g++ -O3 -std=c++17 -fopenmp -fPIC -shared -Wall -o $@ sctools_amd/csrc/csvfmt.cpp -lz

oracle/liboracle.so: oracle/sct_oracle.c include/sctools_gpu.h
	$(MAKE) -s -C oracle liboracle.so

# std::hash<std::string> itself, for tests/test_fastq_process_cpu.py
tests/native/libstdhash.so: tests/native/stdhash.cpp
	g++ -O2 -std=c++17 -fPIC -shared -o $@ tests/native/stdhash.cpp

# the six-digit text round trip of tsmetrics.h on the host, beside glibc's (tests/test_tagsort_native_cpu.py)
tests/native/libtsround.so: tests/native/tsround.cpp sctools_amd/csrc/tsround.h
	g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared -o $@ tests/native/tsround.cpp

# the CRC-32 of fqinflate.h (slices, fold) on the host, beside zlib's (tests/test_fastq_bgzf_cpu.py)
tests/native/libfqcrc.so: tests/native/fqcrc.cpp sctools_amd/csrc/fqinflate.h
	g++ -O2 -std=c++17 -fPIC -shared -Wall -o $@ tests/native/fqcrc.cpp

tests/native/libfxcheck.so: tests/native/fxcheck.cpp sctools_amd/csrc/fixedpt.h
	g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared -o $@ tests/native/fxcheck.cpp

clean:
	rm -f $(ENGINE) $(BAMDEC) $(CSVFMT) $(GBAM) $(BARCODE) $(FASTQ) oracle/liboracle.so tests/native/libfxcheck.so tests/native/libstdhash.so tests/native/libtsround.so tests/native/libfqcrc.so $(SI4)

.PHONY: all clean
