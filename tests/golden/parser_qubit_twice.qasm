OPENQASM 3.0;
include "stdgates.inc";
qubit[3] q;
h q[0];
cx q[0], q[2];
qubit[2] q;
x q[1];
h q[0];
