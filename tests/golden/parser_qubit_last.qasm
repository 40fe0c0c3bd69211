OPENQASM 3.0;
include "stdgates.inc";
qubit[3] q;