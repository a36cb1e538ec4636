#!/bin/bash
# kmer-cnt regression on the small input: runs the MI355X driver on one GPU and compares its "Total k-mers" line with the
# one in the data set's output-reference.txt, like the reference's script of the same name (which has that comparison commented out).
inputs_path="$GENARCH_BENCH_INPUTS_ROOT/kmer-cnt/small"
if [[ -z "$GENARCH_BENCH_INPUTS_ROOT" || ! -d "$inputs_path" ]]; then
    echo "ERROR: You have not set a valid input folder $inputs_path"
    exit 1
fi
scriptfolder="$(dirname "$(realpath "$0")")"
configfolder="$(dirname "$scriptfolder")/config"
binaries_path="$(dirname "$scriptfolder")"
clean=1
job="KMERCNT-REGRESSION-SMALL"
before_command=""
# $GAB_KMERCNT_COMMAND substitutes another binary with the same CLI (e.g. the compiled reference, to run this harness on a box without a GPU)
commands=( "${GAB_KMERCNT_COMMAND:-$binaries_path/kmer-cnt}" )
parallelism=( 'nodes=1, mpi=1, omp=1, gpus=1' )
command_opts="--reads \"$inputs_path/Loman_E.coli_MAP006-1_2D_50x_1000.fasta\" --config \"${GAB_KMERCNT_CONFIG:-$configfolder/raw_reads.cfg}\" --debug --threads \$OMP_NUM_THREADS"
before_run() ( job_name="$1" )
after_run() (
    job_name="$1"
    refkmers="$(grep -m 1 -Eo "Total k-mers [0-9]+" "$inputs_path/output-reference.txt" | cut -d ' ' -f 3)"
    outkmers="$(grep -m 1 -Eo "Total k-mers [0-9]+" "$job_name.err" | cut -d ' ' -f 3)"
    wall_time="$(grep -m 1 "Kernel time:" "$job_name.err" | cut -d ' ' -f 3)"
    if [[ -z "$wall_time" ]]; then echo "Error in the execution"; return 1; fi
    if [[ -z "$outkmers" || "$refkmers" != "$outkmers" ]]; then echo "Reference number of k-mers ($refkmers) != output number of k-mers ($outkmers)"; return 1; fi
    echo "Kernel time: $wall_time s"
    grep "Energy consumption:" "$job_name.err"
    return 0
)
source "$scriptfolder/../../run_wrapper.sh"
